"""blsgpu_signcrypt_share_verify_indexed_batch on the GPU: the case list of tests/signcrypt_indexed_cases.py through the flat call and
TensorOps (both impls, the three schemes, RAW_PROJ under random Z and RAW_AFFINE), and 130 shares in ciphertexts of 1, 0, 31, 33, 0 and
65 shares on every plan of the call -- the row-wide engine apart, which the case list runs on: one wave per share, the lane-split
kernels, and those in chunks of 64.  Expected statuses are the model's (the precedence of the indexed calls on top of
signcrypt_cases.Case.share_status, which tests/test_signcrypt_cases.py and tests/test_signcrypt_indexed_cases.py hold against the
oracle's pairings), and the by-value call's on the gathered keys wherever the position names a valid entry.  The launch counts of the
profile say which pairing / line kernel ran, so no test passes by falling back.  Knobs are read once per process: those runs go
through tests/signcrypt_indexed_worker.py, one attempt each, with its own time limit."""
import ctypes
import json
import os
import pickle
import random
import subprocess
import sys

import pytest

import signcrypt_cases as sc
import signcrypt_indexed_cases as ic
import test_gpu_signcrypt as tg
import util
from util import ref

pytestmark = pytest.mark.gpu

R = sc.R
OK, INVALID, E_ARG, BAD_ENCODING = ic.OK, ic.INVALID_DECRYPTION_SHARE, ic.E_ARG, ic.BAD_ENCODING
SIZES = (1, 0, 31, 33, 0, 65)                     # ciphertext borders inside a wave, on a workgroup border and across it
VALID = (ic.P23_1, ic.P23_2, ic.P23_3, ic.OTHER_1, ic.OTHER_2, ic.P917_0)
PLANS = {'one wave': {'BLSGPU_WIDE_MAX': '0'},
         'lane split': {'BLSGPU_COOP_MAX': '0'},
         'lane split, chunked': {'BLSGPU_COOP_MAX': '0', 'BLSGPU_AB_KNOBS': '1', 'BLSGPU_MILLER_CHUNK': '64'}}


def run_worker(tmp_path, name, env, sets, calls, timeout=240):
    """one attempt: a worker that dies by a signal or outlives its limit fails the test, and nothing further is started"""
    path = str(tmp_path / (name + '.pickle'))
    with open(path, 'wb') as f:
        pickle.dump({'sets': sets, 'calls': calls}, f)
    keep = {k: v for k, v in os.environ.items() if not k.startswith('BLSGPU_') or k == 'BLSGPU_LIB'}
    r = subprocess.run([sys.executable, os.path.join(util.ROOT, 'tests', 'signcrypt_indexed_worker.py'), path], env=dict(keep, **env),
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (name, env, r.returncode, r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def profiled(api, fn):
    """fn() with the profile on: (result, {kernel: launches of this call})"""
    api.profile_enable(True)
    try:
        before = {k: v[1] for k, v in api.profile_read().items()}
        out = fn()
        now = {k: v[1] for k, v in api.profile_read().items()}
    finally:
        api.profile_enable(False)
    return out, {k: now[k] - before.get(k, 0) for k in now if now[k] != before.get(k, 0)}


def affine_ct(sg, ct):
    u, v, w = ct
    return tg.affine(sg, True, u), v, tg.affine(sg, False, w)


# ------------------------------------------------------------------ 1. the case list, on default knobs
@pytest.mark.parametrize('sg', [1, 2])
def test_case_list_flat_call(api, sg):
    """one call per call scheme and format; the statuses of the model, and of the by-value call on the gathered keys wherever the
    position names a valid entry"""
    t = ic.table(sg)
    rng = random.Random(40 + sg)
    with api.KeySet.create(sg, t['blobs'], api.FMT_COMPRESSED, lines=(sg == 1)) as ks:
        assert ks.statuses == t['status']
        for scheme, cl in sorted(ic.by_call_scheme(sg).items()):
            want = [x.expected() for x in cl]
            cts = [sc.raw_ct(x.cs, rng) for x in cl]
            got = api.signcrypt_share_verify_indexed_batch(scheme, ks, cts, [ic.raw_shares(x, rng) for x in cl])
            assert got == want, [(x.name, g, w) for x, g, w in zip(cl, got, want) if g != w]
            acts = [affine_ct(sg, sc.raw_ct(x.cs)) for x in cl]
            ash = [[(pos, tg.affine(sg, True, p)) for pos, p in ic.raw_shares(x)] for x in cl]
            assert api.signcrypt_share_verify_indexed_batch(scheme, ks, acts, ash, fmt=api.FMT_RAW_AFFINE) == want
            # the by-value call with the keys the positions name (a share whose position names none is left out of it)
            gath = [ic.gathered(x, rng) for x in cl]
            byv = api.signcrypt_share_verify_batch(sg, scheme, cts, [[p for p in g if p is not None] for g in gath])
            for x, g, row, b in zip(cl, gath, got, byv):
                assert [s for s, p in zip(row, g) if p is not None] == b, x.name
        assert {s for x in ic.cases(sg) for s in x.expected()} == {OK, INVALID, E_ARG, BAD_ENCODING}


@pytest.mark.parametrize('sg', [1, 2])
def test_case_list_tensor_ops(api, sg):
    """device-resident inputs, a device status"""
    import torch
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    t = ic.table(sg)
    tens = lambda b: torch.tensor(list(b), dtype=torch.uint8, device=dev)
    i64 = lambda xs: torch.tensor(xs, dtype=torch.int64, device=dev)
    with api.KeySet.create(sg, t['blobs'], api.FMT_COMPRESSED, lines=(sg == 1)) as ks:
        for scheme, cl in sorted(ic.by_call_scheme(sg).items()):
            cts = [sc.raw_ct(x.cs) for x in cl]
            voffs, soffs = [0], [0]
            for (_, v, _), x in zip(cts, cl):
                voffs.append(voffs[-1] + len(v))
                soffs.append(soffs[-1] + len(x.shares))
            sh = [p for x in cl for p in ic.raw_shares(x)]
            idx = torch.tensor([pos - 2 ** 32 if pos >= 2 ** 31 else pos for pos, _ in sh], dtype=torch.int32, device=dev)
            us, ws, vs = tens(b''.join(u for u, _, _ in cts)), tens(b''.join(w for _, _, w in cts)), tens(b''.join(v for _, v, _ in cts) or b'\0')
            st = ops.signcrypt_share_verify_indexed_batch(ks, scheme, idx, us, ws, vs, i64(voffs), len(cl), tens(b''.join(p for _, p in sh)), i64(soffs), len(sh))
            assert st.is_cuda and st.cpu().tolist() == [s for x in cl for s in x.expected()], scheme


def test_wrapper_types(api):
    """SignDecryptionShares with member positions over a KeySet, under the Basic DST as SignDecryptionShare.verify"""
    for sg, impl in ((1, api.Bls12381G1Impl), (2, api.Bls12381G2Impl)):
        t = ic.table(sg)
        cl = [x for x in ic.cases(sg) if x.name in ('basic, 3 of 2-of-3', 'tampered share', 'positions past the end', 'aug, 2 of 2-of-3')]
        assert len(cl) == 4
        items = [(api.SignCryptCiphertext(impl, x.cs.scheme, *sc.raw_ct(x.cs)), [(pos, api.SignDecryptionShare(impl, 1 + k, p))
                                                                                  for k, (pos, p) in enumerate(ic.raw_shares(x))]) for x in cl]
        with api.KeySet.create(sg, t['blobs'], api.FMT_COMPRESSED) as ks:
            got = api.verify_shares_many(ks, items)
            assert api.verify_shares_many(ks, []) == []
        want = [[ic.share_expected(x.cs, t, pos, a, ref.BASIC) for pos, a in x.shares] for x in cl]
        assert [[None if e is None else e.kind for e in row] for row in got] == \
            [[None if s == OK else 'InvalidDecryptionShare' if s == INVALID else api.error_from_status(s).kind for s in row] for row in want]
        aug = [x.name for x in cl].index('aug, 2 of 2-of-3')
        assert set(want[aug]) == {INVALID}                       # an honest share of an Aug ciphertext: the Basic DST quirk


def test_call_level_errors_and_edge_shapes(api):
    lib = api.init()
    sg = 2
    t = ic.table(sg)
    x = ic.cases(sg)[0]
    u, v, w = sc.raw_ct(x.cs)
    (pos, a), = ic.raw_shares(x)[:1]
    st = (ctypes.c_int32 * 4)(99, 99, 99, 99)
    off = lambda *xs: ctypes.cast((ctypes.c_uint64 * len(xs))(*xs), ctypes.c_void_p)
    ix = ctypes.cast((ctypes.c_uint32 * 1)(pos), ctypes.c_void_p)
    p, sp = api._ptr, ctypes.cast(st, ctypes.c_void_p)
    with api.KeySet.create(sg, t['blobs'], api.FMT_COMPRESSED) as ks:
        call = lambda h, i, voffs, soffs, n_ct=1, fmt=0, shares=a, status=sp: lib.blsgpu_signcrypt_share_verify_indexed_batch(
            0, h, i, p(u), p(w), p(v), voffs, n_ct, p(shares) if shares else None, soffs, fmt, status)
        assert call(ks.handle, ix, off(0, len(v)), off(0, 1)) == 0 and st[0] == OK
        st[0] = 99
        assert call(ks.handle + 12345, ix, off(0, len(v)), off(0, 1)) == E_ARG                      # an unknown handle
        for voffs, soffs in (((0, len(v)), (1, 1)), ((0, len(v)), (0, 2 ** 32)), ((1, len(v)), (0, 1)), ((0, len(v)), (1, 0))):
            assert call(ks.handle, ix, off(*voffs), off(*soffs)) == E_ARG
        assert call(ks.handle, None, off(0, len(v)), off(0, 1)) == E_ARG                            # a null required argument
        assert call(ks.handle, ix, off(0, len(v)), off(0, 1), shares=None) == E_ARG
        assert call(ks.handle, ix, off(0, len(v)), off(0, 1), status=None) == E_ARG
        assert call(ks.handle, ix, None, off(0, 1)) == E_ARG and call(ks.handle, ix, off(0, len(v)), None) == E_ARG
        assert call(ks.handle, ix, off(0, len(v)), off(0, 1), fmt=api.FMT_COMPRESSED) == E_ARG
        assert st[0] == 99                                                                          # no status was written
        assert call(ks.handle, None, off(0, len(v)), off(0, 0), shares=None, status=None) == 0      # no shares
        assert api.signcrypt_share_verify_indexed_batch(ref.BASIC, ks, [], []) == []
        assert api.signcrypt_share_verify_indexed_batch(ref.BASIC, ks, [(u, v, w)] * 3, [[], [], []]) == [[], [], []]


# ------------------------------------------------------------------ 2. 130 shares on every plan
def batch(sg, sizes, seed, bad_every=None):
    """ciphertexts of the given share counts under the committee's 2-of-3 key, every point from a small pool of scalars (an honest
    share of member j is ks[j] r g).  Failure classes by the share's flat index: the right share under the next member's position,
    an identity share, the identity entry, the invalid entry, positions past the end; bad_every: only a tamper every so many shares.
    Returns (cases, [[(position, a)]], flat expected statuses)."""
    t = ic.table(sg)
    p23 = [sc._scalar(b'p23', sg), sc._scalar(b'p23b', sg)]
    cl, shares, want = [], [], []
    g = 0
    for k, size in enumerate(sizes):
        cs = sc.sealed(sg, 'indexed batch %d / %d' % (seed, k), ref.BASIC, b'message %d' % k, p23, [])
        row = []
        for _ in range(size):
            pos = VALID[g % len(VALID)]
            a = t['ks'][pos] * cs.r % R
            if bad_every:
                if g % bad_every == bad_every // 2:
                    pos = VALID[(g + 1) % len(VALID)]
            elif g % 10 == 3:
                pos = VALID[(g + 1) % len(VALID)]
            elif g % 17 == 5:
                a = 0
            elif g % 23 == 7:
                pos = ic.IDENT
            elif g % 29 == 11:
                pos = ic.BAD
            elif g % 31 == 13:
                pos = ic.N if g % 2 else 2 ** 32 - 1
            row.append((pos, a))
            want.append(ic.share_expected(cs, t, pos, a, ref.BASIC))
            g += 1
        cl.append(cs)
        shares.append(row)
    return cl, shares, want


def raw_batch(sg, cl, shares, aff=False):
    pt = lambda a: tg.affine(sg, True, sc.raw_pk(sg, sc.pk_point(sg, a))) if aff else sc.raw_pk(sg, sc.pk_point(sg, a))
    cts = [affine_ct(sg, sc.raw_ct(cs)) if aff else sc.raw_ct(cs) for cs in cl]
    return cts, [[(pos, pt(a)) for pos, a in row] for row in shares]


def gathered_call(sg, cts, shares, fmt, aff):
    """the by-value call over the shares whose position names a valid entry: (call spec, the flat indices it covers)"""
    t = ic.table(sg)
    key = lambda pos: tg.affine(sg, True, sc.raw_pk(sg, sc.pk_point(sg, t['ks'][pos]))) if aff else sc.raw_pk(sg, sc.pk_point(sg, t['ks'][pos]))
    pairs, covered, g = [], [], 0
    for row in shares:
        out = []
        for pos, p in row:
            if pos < ic.N and t['ks'][pos] is not None:
                out.append((p, key(pos)))
                covered.append(g)
            g += 1
        pairs.append(out)
    return {'sg': sg, 'scheme': ref.BASIC, 'cts': cts, 'pairs': pairs, 'fmt': fmt}, covered


def pairing_launches(got):
    """(tabled one-wave kernels, k_pairing_coop, k_lines2s_tables2, k_lines2s [the shared form counts here: one launch per chunk, the
    general form two], k_group_lines)"""
    return (got.get('k_pairing_coop_tables2', 0) + got.get('k_pairing_coop_rows', 0), got.get('k_pairing_coop', 0), got.get('k_lines2s_tables2', 0),
            got.get('k_lines2s', 0), got.get('k_group_lines', 0))


def expected_launches(plan, tabled, sg, n=130):
    chunks = (n + 63) // 64 if plan == 'lane split, chunked' else 1
    if plan == 'one wave':
        return (1, 0, 0, 0, 1 if tabled and sg == 2 else 0) if tabled else (0, 1, 0, 0, 0)
    if not tabled:
        return (0, 0, 0, 2 * chunks, 0)
    return (0, 0, chunks, 0, 1) if sg == 2 else (0, 0, 0, chunks, 0)


def test_the_130_shares_carry_every_failure_class():
    for sg in (1, 2):
        cl, shares, want = batch(sg, SIZES, 130)
        assert len(want) == 130 and [len(r) for r in shares] == list(SIZES)
        assert set(want) == {OK, INVALID, E_ARG, BAD_ENCODING}
        flat = [s for r in shares for s in r]
        assert any(a == 0 for _, a in flat) and {ic.IDENT, ic.BAD, ic.N, 2 ** 32 - 1} <= {pos for pos, _ in flat}
        for lo, hi in ((0, 1), (1, 32), (32, 65), (65, 130)):
            assert OK in want[lo:hi] and (hi - lo == 1 or INVALID in want[lo:hi])


@pytest.mark.parametrize('knob', ['1', '0'])
@pytest.mark.parametrize('plan', sorted(PLANS))
def test_g2impl_130_shares_on_every_plan(api, tmp_path, plan, knob):
    """Bls12381G2Impl.  BLSGPU_SIGNCRYPT_LINES_MIN=1: the ciphertexts' tables are built (k_group_lines once) and exactly the two-table
    kernel of the plan runs; =0: the general kernels.  The same statuses both times, RAW_PROJ and RAW_AFFINE.  Then, in the same
    process: an identity w in one ciphertext leaves the plan in force for the others; a finite w outside the subgroup whose walk meets
    h = 0 -- (x, 0) -- has no usable rows, and the call runs the general kernels for every share with the by-value statuses"""
    sg = 2
    t = ic.table(sg)
    tabled = knob == '1'
    cl, shares, want = batch(sg, SIZES, 130)
    cts, sh = raw_batch(sg, cl, shares)
    acts, ash = raw_batch(sg, cl, shares, aff=True)
    # identity w in the ciphertext of 31 shares
    iw = list(cl)
    iw[2] = sc.variant(cl[2], 'identity w', w=None)
    want_iw = [ic.share_expected(cs, t, pos, a, ref.BASIC) for cs, row in zip(iw, shares) for pos, a in row]
    assert want_iw[:1] == want[:1] and want_iw[32:] == want[32:] and OK not in want_iw[1:32] and {E_ARG, BAD_ENCODING} & set(want_iw[1:32])
    icts, _ = raw_batch(sg, iw, shares)
    # w = (x, 0) in the ciphertext of 33 shares, RAW_AFFINE
    fcts = list(acts)
    fcts[3] = (acts[3][0], acts[3][1], acts[3][2][:96] + bytes(96))
    byv, covered = gathered_call(sg, fcts, ash, api.FMT_RAW_AFFINE, True)
    sets = {'set': {'sg': sg, 'keys': t['blobs'], 'fmt': api.FMT_COMPRESSED, 'lines': False}}
    ix = lambda c, s, fmt: {'set': 'set', 'scheme': ref.BASIC, 'cts': c, 'shares': s, 'fmt': fmt}
    got = run_worker(tmp_path, 'g2', dict(PLANS[plan], BLSGPU_SIGNCRYPT_LINES_MIN=knob), sets,
                     [ix(cts, sh, api.FMT_RAW_PROJ), ix(acts, ash, api.FMT_RAW_AFFINE), ix(icts, sh, api.FMT_RAW_PROJ), ix(fcts, ash, api.FMT_RAW_AFFINE), byv])['calls']
    for g in got:
        print(plan, knob, g['launches'])
    proj, aff, idw, fall, byvalue = got
    assert proj['st'] == want and aff['st'] == want
    assert pairing_launches(proj['launches']) == expected_launches(plan, tabled, sg)
    assert pairing_launches(aff['launches']) == expected_launches(plan, tabled, sg)
    assert idw['st'] == want_iw
    assert pairing_launches(idw['launches']) == expected_launches(plan, tabled, sg)
    # the fallback: the general kernels whatever the knob says (the row builder ran when the plan asked for tables), the by-value statuses
    assert [fall['st'][i] for i in covered] == byvalue['st']
    assert [s for i, s in enumerate(fall['st']) if not 65 > i >= 32] == [s for i, s in enumerate(want) if not 65 > i >= 32]
    assert OK not in fall['st'][32:65]
    assert pairing_launches(fall['launches'])[:4] == expected_launches(plan, False, sg)[:4]
    assert pairing_launches(fall['launches'])[4] == (1 if tabled else 0)
    assert pairing_launches(byvalue['launches']) == expected_launches(plan, False, sg, len(covered))


@pytest.mark.parametrize('plan', sorted(PLANS))
def test_g1impl_130_shares_on_every_plan(api, tmp_path, plan):
    """Bls12381G1Impl.  Over a set with line rows the pair (w, pk) reads the key's rows and only the share is walked
    (k_pairing_coop_rows; k_lines2s_shared: ONE k_lines2s launch per chunk); over a set without, the general kernels (k_pairing_coop;
    two launches per chunk).  The same statuses both times, RAW_PROJ and RAW_AFFINE"""
    sg = 1
    t = ic.table(sg)
    cl, shares, want = batch(sg, SIZES, 130)
    cts, sh = raw_batch(sg, cl, shares)
    acts, ash = raw_batch(sg, cl, shares, aff=True)
    sets = {name: {'sg': sg, 'keys': t['blobs'], 'fmt': api.FMT_COMPRESSED, 'lines': lines} for name, lines in (('lines', True), ('plain', False))}
    ix = lambda name, c, s, fmt: {'set': name, 'scheme': ref.BASIC, 'cts': c, 'shares': s, 'fmt': fmt}
    res = run_worker(tmp_path, 'g1', PLANS[plan], sets, [ix('lines', cts, sh, api.FMT_RAW_PROJ), ix('lines', acts, ash, api.FMT_RAW_AFFINE),
                                                         ix('plain', cts, sh, api.FMT_RAW_PROJ), ix('plain', acts, ash, api.FMT_RAW_AFFINE)])
    assert res['sets']['lines']['has_lines'] is True and res['sets']['plain']['has_lines'] is False
    for g, name in zip(res['calls'], ('lines', 'lines', 'plain', 'plain')):
        print(plan, name, g['launches'])
        assert g['st'] == want
        assert pairing_launches(g['launches']) == expected_launches(plan, name == 'lines', sg), (name, g['launches'])
        assert g['launches'].get('k_lines2s_keyed', 0) == 0 and g['launches'].get('k_pairing_coop_keyed', 0) == 0


# ------------------------------------------------------------------ 3. default knobs past BLSGPU_COOP_MAX
@pytest.mark.parametrize('sg', [1, 2])
def test_4097_shares_on_default_knobs(api, sg):
    """four ciphertexts, a tamper (the right share under the next member's position) every 97 shares: the statuses equal the pattern;
    Bls12381G1Impl over a set with rows takes the shared line kernel (one k_lines2s launch), Bls12381G2Impl -- more than a thousand
    shares per ciphertext, above the default BLSGPU_SIGNCRYPT_LINES_MIN -- the two-table line kernel"""
    t = ic.table(sg)
    cl, shares, want = batch(sg, (1000, 2000, 97, 1000), 4097, bad_every=97)
    assert len(want) == 4097 and 35 <= want.count(INVALID) <= 45 and set(want) == {OK, INVALID}
    cts, sh = raw_batch(sg, cl, shares)
    with api.KeySet.create(sg, t['blobs'], api.FMT_COMPRESSED, lines=(sg == 1)) as ks:
        got, launches = profiled(api, lambda: api.signcrypt_share_verify_indexed_batch(ref.BASIC, ks, cts, sh))
    flat = [s for g in got for s in g]
    bad = [(i, flat[i], want[i]) for i in range(len(want)) if flat[i] != want[i]][:10]
    assert not bad and len(flat) == 4097, bad
    print(sg, launches)
    assert launches.get('k_millerf2s', 0) == 1 and launches.get('k_pairing_coop', 0) == 0
    if sg == 1:
        assert launches.get('k_lines2s', 0) == 1
    else:
        assert (launches.get('k_lines2s_tables2', 0), launches.get('k_group_lines', 0), launches.get('k_lines2s', 0)) == (1, 1, 0)
