"""Shared-message verify on the GPU (blsgpu_verify_shared_batch, blsgpu_verify_shared_indexed_batch).  Expected statuses are the
oracle's -- one verification per item with its group's message (tests/verify_shared_cases.py; tests/test_verify_shared_cases.py
checks the case list on the CPU) -- and, beyond the oracle's sample of a large batch, the pattern the batch was tampered with.
Runs that need their own process (the knobs are read once) go through tests/verify_shared_worker.py."""
import ctypes
import functools
import json
import os
import pickle
import random
import subprocess
import sys

import pytest

import multi_batch_cases as mb
import util
import verify_shared_cases as vc
from util import ref

pytestmark = pytest.mark.gpu

E_ARG = -3
R = vc.R


@pytest.fixture(scope='module')
def bo():
    return util.load_c_oracle()


def flat(groups_of_statuses):
    return [s for g in groups_of_statuses for s in g]


def aff(group, raw):
    """RAW_PROJ (Z = 1, or the identity) -> RAW_AFFINE"""
    half = 96 * group
    return bytes(half) if mb._coords(group, raw)[2] in (0, (0, 0)) else raw[:half]


# ------------------------------------------------------------------ the case list
@pytest.mark.parametrize('sg,scheme', vc.COMBOS, ids=vc.COMBO_IDS)
def test_case_list(api, pkg, sg, scheme):
    """the C ABI (both raw formats) and verify_shared_many with default knobs: the oracle's status for every item"""
    rng = random.Random(5 * sg + scheme)
    for name, groups, expect in vc.batches(sg, scheme):
        got = flat(api.verify_shared_batch(sg, scheme, vc.raw_groups(sg, groups, rng)))
        print(name, got)
        assert got == expect, name
        z1 = vc.raw_groups(sg, groups)
        affine = [(m, [aff(3 - sg, p) for p in pks], [aff(sg, s) for s in sigs]) for m, pks, sigs in z1]
        assert flat(api.verify_shared_batch(sg, scheme, affine, fmt=api.FMT_RAW_AFFINE)) == expect, name
        impl = pkg.Bls12381G1Impl if sg == 1 else pkg.Bls12381G2Impl
        many = pkg.verify_shared_many([(m, [(pkg.PublicKey(impl, p), pkg.Signature(impl, scheme, s)) for p, s in zip(pks, sigs)]) for m, pks, sigs in z1])
        assert many == [api.error_from_status(st) for st in expect], name
    assert pkg.verify_shared_many([]) == []


# ------------------------------------------------------------------ larger batches: signed on the device, tampered by a pattern
def tamper_kind(i):
    """about one item in ten: 1 = another item's signature, 2 = the identity signature, 3 = the identity key"""
    return {3: 1, 13: 2, 23: 3}.get(i % 30, 0)


@functools.lru_cache(maxsize=None)
def signed_batch(sg, scheme, sizes):
    """(raw groups, the pattern's statuses): group g's items signed under its message by sign_batch, then tampered by tamper_kind"""
    from __graft_entry__ import import_pkg
    api = import_pkg().api
    n = sum(sizes)
    rng = random.Random(n + 7 * sg + scheme)
    msgs = [b'shared message %d of %d' % (g, len(sizes)) if g != 2 else b'' for g in range(len(sizes))]
    item_msg = [msgs[g] for g, s in enumerate(sizes) for _ in range(s)]
    pks, sigs = api.sign_batch(sg, scheme, [rng.randrange(1, R) for _ in range(n)], item_msg)
    expect = []
    orig = list(sigs)
    for i in range(n):
        k = tamper_kind(i)
        if k == 1:
            sigs[i] = orig[(i + 1) % n] if n > 1 else mb.negate(sg, orig[i])
        elif k == 2:
            sigs[i] = mb.identity(sg)
        elif k == 3:
            pks[i] = mb.identity(3 - sg)
        expect.append({0: vc.OK, 1: vc.INVALID_SIGNATURE, 2: vc.SIG_IDENTITY, 3: vc.PK_IDENTITY}[k])
    groups, at = [], 0
    for g, s in enumerate(sizes):
        groups.append((msgs[g], pks[at:at + s], sigs[at:at + s]))
        at += s
    return groups, expect


def oracle_sample(bo, sg, scheme, groups, expect, k=64):
    """the C oracle on k items spread over the batch (all of them when it has no more): they must equal the pattern's statuses"""
    items = [(m, pk, sig) for m, pks, sigs in groups for pk, sig in zip(pks, sigs)]
    n = len(items)
    pick = sorted(set(range(n)) if n <= k else set(random.Random(n).sample(range(n), k - 8)) | {0, 3, 13, 23, n - 1, n - 2, n // 2, n // 2 + 1})
    for i in pick:
        m, pk, sig = items[i]
        assert bo.bo_verify(sg, scheme, pk, sig, m, len(m)) == expect[i], i


LANE_SPLIT_SIZES = (1, 0, 31, 33, 0, 65)        # group borders inside a wave, on a workgroup border and across it


@functools.lru_cache(maxsize=None)
def lane_split_reference(sg):
    """the 130-item input of the table-form tests and the ORACLE's status of every item (computed once, shared by the plans)"""
    groups, expect = signed_batch(sg, ref.POP, LANE_SPLIT_SIZES)
    want = vc.oracle_statuses(util.load_c_oracle(), sg, ref.POP, groups)
    assert want == expect and sum(1 for s in want if s) >= 12
    return groups, want


def run_worker(tmp_path, name, env, calls, timeout=300):
    """one attempt: a worker that dies by a signal or outlives its limit fails the test, and nothing further is started"""
    path = str(tmp_path / (name + '.pickle'))
    with open(path, 'wb') as f:
        pickle.dump({'calls': calls}, f)
    keep = {k: v for k, v in os.environ.items() if not k.startswith('BLSGPU_') or k == 'BLSGPU_LIB'}
    r = subprocess.run([sys.executable, os.path.join(util.ROOT, 'tests', 'verify_shared_worker.py'), path], env=dict(keep, **env),
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (name, env, r.returncode, r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


LANE_SPLIT_PLANS = [
    ('tables', {'BLSGPU_COOP_MAX': '0', 'BLSGPU_SHARED_LINES_MIN': '1'}, True),
    ('no_tables', {'BLSGPU_COOP_MAX': '0', 'BLSGPU_SHARED_LINES_MIN': '0'}, False),
    # a chunk border inside a group: the group lookup must use the item's index in the batch, not in the chunk
    ('tables_chunk_64', {'BLSGPU_COOP_MAX': '0', 'BLSGPU_SHARED_LINES_MIN': '1', 'BLSGPU_AB_KNOBS': '1', 'BLSGPU_MILLER_CHUNK': '64'}, True),
]


@pytest.mark.parametrize('name,env,tables', LANE_SPLIT_PLANS, ids=[p[0] for p in LANE_SPLIT_PLANS])
@pytest.mark.parametrize('sg', [1, 2])
def test_table_form_on_the_lane_split_path(tmp_path, sg, name, env, tables):
    """130 items in groups of 1, 0, 31, 33, 0, 65 on the lane-split kernels: the oracle's statuses with the per-group line tables
    (Bls12381G2Impl: k_group_lines must have run, so the test cannot pass by falling back), without them (it must not have run),
    and with 64-item chunks.  Bls12381G1Impl shares the hash only: no table either way."""
    groups, want = lane_split_reference(sg)
    got = run_worker(tmp_path, name, env, [{'sg': sg, 'scheme': ref.POP, 'groups': groups, 'fmt': 0}])[0]
    print(name, got['launches'])
    assert got['st'] == want
    assert got['launches'].get('k_prepare_shared', 0) >= 2              # k_group_affine and k_prepare_shared
    assert got['launches'].get('k_millerf2s', 0) == (3 if 'chunk' in name else 1)
    if tables and sg == 2:
        assert got['launches'].get('k_group_lines', 0) == 1 and got['launches'].get('k_lines2s', 0) == (3 if 'chunk' in name else 1)
    else:
        assert got['launches'].get('k_group_lines', 0) == 0
        assert got['launches'].get('k_lines2s', 0) == (3 if 'chunk' in name else 1) * (2 if sg == 2 else 1)


SIZE_CASES = [(n, 3) for n in (1, 64, 513, 1025)] + [(4097, 5)]


@pytest.mark.parametrize('n,n_groups', SIZE_CASES, ids=[str(n) for n, _ in SIZE_CASES])
@pytest.mark.parametrize('sg', [1, 2])
def test_every_size_branch(api, bo, sg, n, n_groups):
    """default knobs, every size the host branches on: the row-wide engine (1, 64), one wave per item (513, 1,025) and -- past
    BLSGPU_COOP_MAX -- the lane-split kernels (4,097 items in 5 groups; their table form is driven by the plans above); unequal
    groups, one of them with the empty message"""
    cut = sorted({n * k // n_groups + (k % 2) for k in range(1, n_groups)} & set(range(n + 1)))
    sizes = tuple(b - a for a, b in zip([0] + cut, cut + [n]))
    sizes = sizes + (0,) * (n_groups - len(sizes))
    assert sum(sizes) == n and len(sizes) == n_groups
    groups, expect = signed_batch(sg, ref.POP, sizes)
    oracle_sample(bo, sg, ref.POP, groups, expect)
    got = flat(api.verify_shared_batch(sg, ref.POP, groups))
    bad = [(i, got[i], expect[i]) for i in range(n) if got[i] != expect[i]][:10]
    assert not bad and len(got) == n, bad


@pytest.mark.parametrize('sg,scheme', [(1, ref.AUG), (2, ref.AUG), (2, ref.BASIC)], ids=['g1-aug', 'g2-aug', 'g2-basic'])
def test_other_schemes_at_a_middle_size(api, bo, sg, scheme):
    """MessageAugmentation copies the messages out per item (600 items: past the row-wide engine); Basic differs in the DST only"""
    groups, expect = signed_batch(sg, scheme, (200, 0, 399, 1))
    oracle_sample(bo, sg, scheme, groups, expect, k=24)
    assert flat(api.verify_shared_batch(sg, scheme, groups)) == expect


# ------------------------------------------------------------------ registered key sets
N_KEYS, IDENT, BAD = 40, 5, 11


@pytest.mark.parametrize('tables', [False, True], ids=['plain', 'keyset_tables'])
@pytest.mark.parametrize('sg', [1, 2])
def test_indexed(api, sg, tables):
    """a table of 40 keys with one identity entry and one that does not decode: the statuses of the by-value call on the keys the set
    hands out, except where the key-set precedence applies (an index outside the table, then the entry's creation status)"""
    g = 3 - sg
    rng = random.Random(50 + sg)
    ks = [rng.randrange(1, R) for _ in range(N_KEYS)]
    blobs = api.serialize(g, mb.key_points(api, sg, ks))
    w = len(blobs[0])
    ks[IDENT], blobs[IDENT] = 0, b'\xc0' + bytes(w - 1)
    ks[BAD], blobs[BAD] = None, bytes([blobs[BAD][0] & 0x9f | 0x1f]) + b'\xff' * (w - 1)
    valid = [i for i, k in enumerate(ks) if k]
    sizes = [0, 7, 1, 0, 40, 22]
    msgs = [b'indexed %d' % s for s in range(len(sizes))]
    idx = [[rng.choice(valid) for _ in range(s)] for s in sizes]
    idx[1][2], idx[1][3] = valid[0], valid[1]
    with api.KeySet.create(sg, blobs, tables=tables) as kset:
        assert kset.info()['has_tables'] == tables and kset.statuses[BAD] == api.BAD_ENCODING
        flat_idx = [i for ix in idx for i in ix]
        item_msg = [msgs[s] for s, ix in enumerate(idx) for _ in ix]
        sigs = mb.signatures(api, sg, ref.POP, [ks[i] for i in flat_idx], item_msg)
        at = [sum(sizes[:s]) for s in range(len(sizes))]
        # group 1: a signature of the next item; group 4: the identity entry, the invalid entry, two positions outside the table, an identity signature
        sigs[at[1] + 2] = sigs[at[1] + 3]
        idx[4][3], idx[4][9], idx[4][17], idx[4][39], sigs[at[4] + 20] = IDENT, BAD, N_KEYS, 2 ** 32 - 1, mb.identity(sg)
        sigs[at[4] + 17] = mb.identity(sg)                  # ... and one of them under an identity signature: the index still decides
        groups = [(msgs[s], idx[s], sigs[at[s]:at[s] + sizes[s]]) for s in range(len(sizes))]
        got = api.verify_shared_indexed_batch(kset, ref.POP, groups)
        inside = [[i if i < N_KEYS else valid[0] for i in ix] for ix in idx]
        want = api.verify_shared_batch(sg, ref.POP, [(m, kset.get(ix)[0] if ix else [], s) for (m, _, s), ix in zip(groups, inside)])
        want[4][9], want[4][17], want[4][39] = api.BAD_ENCODING, E_ARG, E_ARG
        assert got == want
        assert [len(x) for x in got] == sizes and got[1] == [0, 0, 1, 0, 0, 0, 0] and got[2] == [0]
        assert got[4][3] == api.PK_IDENTITY and got[4][20] == api.SIG_IDENTITY and set(got[5]) == {0}
        assert sum(1 for s in got[4] if s == 0) == 35
        assert api.verify_shared_indexed_batch(kset, ref.POP, []) == []
        dead = kset.handle
    st = (ctypes.c_int32 * 4)(-7, -7, -7, -7)
    offs = (ctypes.c_uint64 * 2)(0, 1)
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    assert api.init().blsgpu_verify_shared_indexed_batch(0, dead, p(offs), p(offs), p(offs), 1, p(offs), p(offs), 0, p(st)) == E_ARG
    assert list(st) == [-7] * 4


# ------------------------------------------------------------------ arguments
def test_argument_errors_write_no_status(api):
    lib = api.init()
    groups, _ = signed_batch(2, ref.POP, (2, 1))
    pkb, sgb = b''.join(p for g in groups for p in g[1]), b''.join(s for g in groups for s in g[2])
    blob = b''.join(g[0] for g in groups)
    moffs = [0, len(groups[0][0]), len(blob)]
    st = (ctypes.c_int32 * 3)(-7, -7, -7)
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    u64 = lambda v: (ctypes.c_uint64 * len(v))(*v)  # noqa: E731

    def call(ioffs, mo=moffs, fmt=0, sg=2, scheme=ref.POP, n_groups=2):
        return lib.blsgpu_verify_shared_batch(sg, scheme, api._ptr(pkb), api._ptr(sgb), p(u64(ioffs)), n_groups, api._ptr(blob), p(u64(mo)), fmt, p(st))
    assert call([0, 3, 2]) == E_ARG                               # decreasing item offsets
    assert call([1, 2, 3]) == E_ARG                               # ... that do not start at 0
    assert call([0, 2, 3], mo=[0, moffs[2], moffs[1]]) == E_ARG   # decreasing message offsets
    assert call([0, 2, 3], mo=[1, moffs[1], moffs[2]]) == E_ARG
    assert call([0, 2, 3], fmt=api.FMT_COMPRESSED) == E_ARG and call([0, 2, 3], fmt=api.FMT_LEGACY) == E_ARG      # wire formats
    assert call([0, 2, 3], sg=3) == E_ARG and call([0, 2, 3], scheme=3) == E_ARG
    assert call([0, 2, 2 ** 32]) == E_ARG                         # 2^32 items
    assert lib.blsgpu_verify_shared_batch(2, ref.POP, None, None, None, 2, None, None, 0, None) == E_ARG
    assert list(st) == [-7, -7, -7]
    assert lib.blsgpu_verify_shared_batch(2, ref.POP, None, None, None, 0, None, None, 0, None) == 0                   # no groups
    assert call([0, 0, 0]) == 0 and list(st) == [-7, -7, -7]      # no items
    assert call([0, 2, 3]) == 0 and list(st) == [0, 0, 0]


@pytest.mark.parametrize('sg', [1, 2])
def test_device_pointers(api, sg):
    """keys, signatures, both offset arrays, messages and the statuses on the device (TensorOps), by value and over a key set"""
    import torch
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    groups, expect = signed_batch(sg, ref.POP, (1, 0, 31, 33, 0, 65))
    tens = lambda b: torch.tensor(list(b), dtype=torch.uint8, device=dev)  # noqa: E731
    i64 = lambda v: torch.tensor(list(v), dtype=torch.int64, device=dev)  # noqa: E731
    ioffs, moffs = [0], [0]
    for m, pks, _ in groups:
        ioffs.append(ioffs[-1] + len(pks))
        moffs.append(moffs[-1] + len(m))
    n = ioffs[-1]
    pk_t, sig_t = tens(b''.join(p for g in groups for p in g[1])), tens(b''.join(s for g in groups for s in g[2]))
    msg_t = tens(b''.join(g[0] for g in groups))
    st = ops.verify_shared_batch(sg, ref.POP, pk_t, sig_t, i64(ioffs), len(groups), msg_t, i64(moffs), n)
    assert st.device == dev and st.dtype == torch.int32 and st.cpu().tolist() == expect
    keys = [p for g in groups for p in g[1]]
    with api.KeySet.create(sg, keys, api.FMT_RAW_PROJ) as kset:
        idx = torch.arange(n, dtype=torch.int32, device=dev)
        st = ops.verify_shared_indexed_batch(kset, ref.POP, idx, sig_t, i64(ioffs), len(groups), msg_t, i64(moffs), n)
        assert st.device == dev and st.cpu().tolist() == expect
