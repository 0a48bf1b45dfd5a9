"""The row-wide engine (csrc/wide.cuh, csrc/wide_engine.cuh, the tables of csrc/wide_tables.cuh) ON THE DEVICE, operation by operation:
every one of the 37 operations of table set F12, the 42 of set PT and the built-in FPINV through blsgpu_debug_wide_steps, which runs any
table operation on caller-supplied limbs, one 256-thread workgroup per item.

The runs are those of tests/wide_cases.py (tests/test_wide_cases.py proves the inputs legal and the checker sharp without a GPU): per
operation and per aliasing shape in which the generated programs use it, ONE door call that carries every input class as its items --
random elements, zeros, ones, values just inside +-0.6 p on extreme limb patterns, the aligned item that takes the widest product row to
2^61.7 of its 2^62, products whose Montgomery quotient digits are all maximal -- with the whole value store read back: every output is
congruent to tests/wide_tables_check.py sim_program on integers (exact, no tolerance) and inside the output contract, and nothing but the
destinations (and the product scratch) changed.  Then real step sequences, chains, the whole PAIR_GENERAL program, the fill word, item
counts, and the door's refusals."""
import pytest

import wide_cases as wc

pytestmark = pytest.mark.gpu

OPS = ['%s:%s' % x for x in wc.ALL_OPS]
_done = set()


def launch(api, run, items=None, fill=0, out_idx=None):
    """the whole store (or the values out_idx names) of every item"""
    ts = wc.SETS[run['set']]
    its = run['items'] if items is None else [run['items'][i] for i in items]
    return api.debug_wide_steps(ts.number, ts.words(run['steps']), run['in_idx'], its, list(range(ts.nv)) if out_idx is None else out_idx, fill, run['reps'])


def run_and_check(api, run, items=None, fill=0):
    idx = list(range(len(run['items']))) if items is None else list(items)
    stores = launch(api, run, idx, fill)
    assert len(stores) == len(idx)
    for i, st in zip(idx, stores):
        wc.check(run, i, st, fill)
    _done.update((run['set'], n) for n in run['ops'])
    return stores


@pytest.mark.parametrize('op', OPS)
def test_operation(api, op):
    """every input class, every aliasing shape of the programs; the stores of a second launch are the same words"""
    for run in wc.op_runs(*op.split(':')):
        first = run_and_check(api, run)
        assert launch(api, run) == first, '%s: two launches differ' % run['name']


@pytest.mark.parametrize('op', OPS)
def test_fill_and_item_counts(api, op):
    """fill words 0, 0xffffffff, 0x7fffffff under the values the operation does not read: right each time, and outside the product
    scratch the destinations hold the same limbs; then 1, 2 and 5 workgroups with different items"""
    for run in wc.op_runs(*op.split(':')):
        wr = sorted(wc.written(run))
        outs = [[[st[v] for v in wr] for st in run_and_check(api, run, fill=f)] for f in wc.FILLS]
        assert outs[0] == outs[1] == outs[2], '%s: the result depends on the fill' % run['name']
        n_items = len(run['items'])
        for k, n in enumerate(wc.COUNTS):
            run_and_check(api, run, [(7 * k + 3 * j) % n_items for j in range(n)], fill=wc.FILLS[k])


@pytest.mark.parametrize('k', range(len(wc.sequence_runs())))
def test_sequences(api, k):
    """verbatim slices of the generated programs -- a Miller doubling and addition step of both pairs with line scaling and MUL_LINE, a
    sixteen-point sum of each group, the G2 cofactor clearing, the isogeny chain -- on the largest coordinates and on random points:
    the whole store against sim_program"""
    run_and_check(api, wc.sequence_runs()[k])


@pytest.mark.parametrize('k', range(len(wc.chain_runs())))
def test_chains(api, k):
    """reps = 2 and 17: MUL and SQR with an aliased accumulator, CYC_SQR on cyclotomic elements, PDBL1 PDBL2 on a point"""
    run_and_check(api, wc.chain_runs()[k])


def test_whole_pairing_program(api):
    """PAIR_GENERAL once, a valid and an invalid signature on two workgroups: T, and every other value the program writes, against the
    simulator; T is one exactly for the valid signature"""
    run, want_one = wc.pairing_run()
    stores = run_and_check(api, run)
    ts = wc.SETS['F12']
    t = ts.lay.base['T']
    for st, one in zip(stores, want_one):
        f = wc.chk.unflat([wc.elem_of(st[t + k][:wc.NL]) for k in range(12)])
        assert (f == wc.c.F12_ONE) == one


def test_refusals(api):
    """the host refuses, with BLSGPU_E_ARG and without a launch, every program that could wait on a partner or leave the value store"""
    f12, pt = wc.SETS['F12'], wc.SETS['PT']
    one = [[[0] * 16]]                                                  # one item, one input value

    def refused(ts, steps, in_idx=(0,), out_idx=(0,), items=one, reps=1):
        with pytest.raises(api.BlsGpuRuntimeError, match=r'rc=-3:'):              # BLSGPU_E_ARG
            api.debug_wide_steps(ts.number, steps, list(in_idx), items, list(out_idx), 0, reps)

    F, T = f12.lay.base['F'], f12.lay.base['T']
    for name in wc.HANDOVER:                                            # the hand-over built-ins, whatever their arguments
        refused(f12, [(f12.ids[name], 0, 4, 0)])
        refused(f12, [(f12.ids[name], T, 0, 0)])
        refused(f12, [(f12.ids['COPY'], T, F, F), (f12.ids[name], T, 0, 0)])
    refused(f12, [(f12.ids['PUBF'] + 1, T, F, F)])                      # past the table and the built-ins
    refused(f12, [(0xffff, T, F, F)])
    refused(pt, [(len(pt.ops), 0, 0, 0)])                               # FPINV's number in a set that has none
    refused(pt, [(len(pt.ops) + 1, 0, 0, 0)])
    # a reference whose extent passes NV: dst, a and b in turn (MUL reads and writes twelve values), and a bare index past the store
    for d, a, b in ((f12.nv - 11, F, F), (T, f12.nv - 11, F), (T, F, f12.nv - 11), (f12.nv, F, F), (T, F, 0xffff)):
        refused(f12, [(f12.ids['MUL'], d, a, b)])
    api.debug_wide_steps(0, [(f12.ids['COPY'], f12.nv - 12, f12.nv - 12, F)], [f12.nv - 1], one, [f12.nv - 1], 0)      # the last twelve values are fine
    refused(f12, [(f12.ids['FPINV'], f12.nv, F, F)])
    refused(f12, [(f12.ids['FPINV'], T, f12.nv, F)])
    last = pt.lay.base['ISO']
    refused(pt, [(pt.ids['C2NEG'], pt.nv - 5, last, last)])
    # len > PROG_MAX, and an empty program
    pmax = {ts.name: max(len(p) for p in ts.programs.values()) for ts in (f12, pt)}
    refused(f12, [(f12.ids['COPY'], T, F, F)] * (pmax['F12'] + 1))
    refused(pt, [(pt.ids['C2NEG'], last, last, last)] * (pmax['PT'] + 1))
    refused(f12, [])
    # value indices past the store, no items, a table set that does not exist
    refused(f12, [(f12.ids['COPY'], T, F, F)], in_idx=(f12.nv,))
    refused(f12, [(f12.ids['COPY'], T, F, F)], out_idx=(f12.nv,))
    refused(f12, [(f12.ids['COPY'], T, F, F)], items=[])
    refused(f12, [(f12.ids['COPY'], T, F, F)], reps=0)
    with pytest.raises(api.BlsGpuRuntimeError, match=r'rc=-3:'):
        api.debug_wide_steps(2, [(0, 0, 0, 0)], [0], one, [0], 0)


def test_every_operation_was_exercised(api):
    """coverage is a condition: the operations run above are the generator's OPS plus OPS_PT plus FPINV, minus the hand-over built-ins --
    a new table operation without cases fails here (and in tests/test_wide_cases.py)"""
    for s, n in wc.ALL_OPS:                   # under a test selection: whatever was not reached above runs now
        if (s, n) not in _done:
            for run in wc.op_runs(s, n):
                run_and_check(api, run, items=range(0, len(run['items']), 5))
    want = {('F12', o.name) for o in wc.g.OPS} | {('PT', o.name) for o in wc.g.OPS_PT} | {('F12', 'FPINV')}
    assert _done == want and len(want) == 80
