"""Registered key sets on the GPU (blsgpu_keyset_*, the *_indexed_batch entry points).  Expected results come from closed-form valid
sets (tests/keyset_cases.py), from the Python oracle's scalar multiplication, and from the non-indexed entry points run on the keys
that KeySet.get hands out."""
import ctypes
import json
import os
import random
import subprocess
import sys

import pytest

import keyset_cases as kc
import keyset_single_worker as single
import util
from util import c

pytestmark = pytest.mark.gpu

E_ARG = -3
COMBOS = [(1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)]
COMBO_IDS = ['g1-basic', 'g1-aug', 'g1-pop', 'g2-basic', 'g2-aug', 'g2-pop']


@pytest.fixture(scope='module')
def sets_of(api):
    """(sg, tables) -> a KeySet created from the Modern wire blobs of kc.table; closed when the module is done"""
    made = {}

    def get(sg, tables):
        if (sg, tables) not in made:
            t = kc.table(api, sg)
            made[sg, tables] = api.KeySet.create(sg, t['blobs'], t['fmt'], tables=tables)
            assert made[sg, tables].info()['has_tables'] == tables
        return made[sg, tables]

    yield get
    for ks in made.values():
        ks.close()


@pytest.mark.parametrize('sg', [1, 2])
def test_create_get_info(api, sg):
    g = 3 - sg
    half = 96 * g
    for legacy in ([False, True] if sg == 2 else [False]):
        t = kc.table(api, sg, legacy)
        with api.KeySet.create(sg, t['blobs'], t['fmt'], tables=legacy) as ks:
            assert ks.statuses == t['status']
            info = ks.info()
            assert (info['sig_group'], info['n'], info['has_tables']) == (sg, kc.N, legacy) and info['device_bytes'] >= kc.N * (144 * g + 4)
            everything = list(range(kc.N))
            ok = [i for i in everything if t['status'][i] == 0]
            want = api.serialize(g, [t['points'][i] for i in ok], legacy=legacy)
            for fmt in (api.FMT_RAW_PROJ, api.FMT_RAW_AFFINE, api.FMT_COMPRESSED) + ((api.FMT_LEGACY,) if sg == 2 else ()):
                out, st = ks.get(everything, fmt)
                assert st == t['status']
                if fmt == api.FMT_RAW_AFFINE:
                    assert out[kc.IDENT] == bytes(half) and out[kc.BAD] == bytes(half)
                    proj = [o + util.fp_raw(1) + (util.fp_raw(0) if g == 2 else b'') for o in out]
                    proj[kc.IDENT] = kc.mb.identity(g)
                    got = api.serialize(g, [proj[i] for i in ok], legacy=legacy)
                elif fmt == api.FMT_RAW_PROJ:
                    got = api.serialize(g, [out[i] for i in ok], legacy=legacy)
                else:
                    got = [out[i] for i in ok]
                    if (fmt == api.FMT_LEGACY) != legacy:
                        got = api.serialize(g, api.deserialize(g, got, legacy=fmt == api.FMT_LEGACY)[0], legacy=legacy)
                assert got == want, fmt
            assert ks.get([kc.DUP_A], api.FMT_COMPRESSED)[0] == ks.get([kc.DUP_B], api.FMT_COMPRESSED)[0]
            assert ks.get([], api.FMT_COMPRESSED) == ([], [])
            with pytest.raises(api.BlsGpuRuntimeError):
                ks.get([0, kc.N])
    # raw formats are taken as they are; every status is OK
    t = kc.table(api, sg)
    pts = [kc.mb.identity(g) if s else p for p, s in zip(t['points'], t['status'])]
    aff = [bytes(half) if k in (0, None) else p[:half] for p, k in zip(pts, t['ks'])]
    for fmt, raws in ((api.FMT_RAW_PROJ, pts), (api.FMT_RAW_AFFINE, aff)):
        with api.KeySet.create(sg, raws, fmt) as ks:
            assert ks.statuses == [0] * kc.N
            assert ks.get(list(range(kc.N)), api.FMT_COMPRESSED)[0] == api.serialize(g, pts)


def test_stale_handles_and_other_calls_keep_working(api):
    lib = api.init()
    t = kc.table(api, 2)
    ks = api.KeySet.create(2, t['blobs'], t['fmt'])
    dead = ks.handle
    ks.close()
    ks.close()                                           # closing twice is harmless
    buf = ctypes.create_string_buffer(4096)
    st = (ctypes.c_int32 * 4)()
    idx = (ctypes.c_uint32 * 4)(0, 1, 2, 3)
    offs = (ctypes.c_uint64 * 3)(0, 2, 4)
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    for h in (0, dead, dead + 1000, 2 ** 64 - 1):
        assert lib.blsgpu_keyset_destroy(h) == E_ARG
        assert lib.blsgpu_keyset_info(h, None, None, None, None) == E_ARG
        assert lib.blsgpu_keyset_get(h, p(idx), 4, 0, p(buf), p(st)) == E_ARG
        assert lib.blsgpu_keyset_mul(h, p(idx), p(buf), 4, p(buf)) == E_ARG
        assert lib.blsgpu_multi_verify_indexed_batch(0, h, p(idx), p(offs), 2, p(buf), p(buf), p(offs), 0, p(st)) == E_ARG
        assert lib.blsgpu_verify_secure_indexed_batch(0, h, p(idx), p(offs), 2, p(buf), p(buf), p(offs), 0, 0, p(st)) == E_ARG
        assert lib.blsgpu_sum_indexed_batch(h, p(idx), p(offs), 2, p(buf)) == E_ARG
        assert lib.blsgpu_verify_indexed_batch(0, h, p(idx), p(buf), p(buf), p(offs), 2, 0, p(st)) == E_ARG
    with pytest.raises(api.BlsGpuRuntimeError, match='key set'):
        api.KeySet(dead, None).info()
    pks, sigs = api.sign_batch(2, 0, [3, 4], [b'a', b'b'])
    assert api.verify_batch(2, 0, pks, sigs, [b'a', b'c']) == [api.OK, api.INVALID_SIGNATURE]


@pytest.mark.parametrize('tables', [False, True], ids=['ladder', 'tables'])
@pytest.mark.parametrize('sg', [1, 2])
def test_mul(api, sets_of, sg, tables):
    """scalar times entry against the oracle's double-and-add on the generator entry, and against blsgpu_msm with n = 1 everywhere"""
    g = 3 - sg
    t, ks = kc.table(api, sg), sets_of(sg, tables)
    rng = random.Random(40 + sg)
    rand_key = t['valid'][17]
    pairs = [(i, s) for i in (kc.GEN, rand_key, kc.IDENT, kc.BAD) for s in kc.SPECIAL_SCALARS]
    pairs += [(rng.choice(t['valid']), rng.randrange(2 ** 256)) for _ in range(64)]
    assert len(pairs) > 65                                # more than one workgroup
    out = ks.mul([i for i, _ in pairs], [s for _, s in pairs])
    got = api.serialize(g, out)
    ident = api.serialize(g, [kc.mb.identity(g)])[0]
    E, gen, comp = (c.E1, c.G1_GEN, c.g1_compress) if g == 1 else (c.E2, c.G2_GEN, c.g2_compress)
    for (i, s), b, raw in zip(pairs, got, out):
        if i in (kc.IDENT, kc.BAD) or s % kc.R == 0:
            assert b == ident, (i, s)
        elif i == kc.GEN:
            assert b == comp(E.mul(gen, s % kc.R)), hex(s)
    pts = ks.get([i for i, _ in pairs])[0]
    for (i, s), p, b in zip(pairs, pts, got):
        assert api.serialize(g, [api.point_sum(g, [p], [s])])[0] == b, (i, hex(s))
    with pytest.raises(api.BlsGpuRuntimeError):
        ks.mul([1, 2 ** 32 - 1], [1, 1])


@pytest.mark.parametrize('sg,scheme', COMBOS, ids=COMBO_IDS)
def test_indexed_multi_sum_single(api, sets_of, sg, scheme):
    g = 3 - sg
    t = kc.table(api, sg)
    sets = kc.multi_sets(api, sg, scheme, t, random.Random(7 * sg + scheme))
    bad = kc.tampered(api, sg, sets)
    ks = sets_of(sg, False)
    st = api.multi_verify_indexed_batch(ks, scheme, sets)
    assert st == [api.SIG_IDENTITY] + [api.OK] * (len(sets) - 1)
    got = api.multi_verify_indexed_batch(ks, scheme, bad)
    want = api.multi_verify_batch(sg, scheme, kc.gathered(api, ks, bad))
    print('indexed', got, 'by value', want)
    assert got == want and len(set(want)) >= 4
    assert api.multi_verify_indexed_batch(sets_of(sg, True), scheme, sets + bad) == st + want       # tables change nothing
    # the sums: the same group elements as blsgpu_sum_batch gives for the gathered keys
    idxs = [s[0] for s in sets + bad]
    sums = api.sum_indexed_batch(ks, idxs)
    assert api.serialize(g, sums) == api.serialize(g, api.sum_batch(g, [ks.get(i)[0] for i in idxs]))
    assert sums[0] == bytes(144 * g)
    # one key per item
    n = 70
    rng = random.Random(90 + sg)
    idx = [rng.choice(t['valid']) for _ in range(n)]
    msgs = [b'item %d' % i for i in range(n)]
    sigs = kc.mb.signatures(api, sg, scheme, [t['ks'][i] for i in idx], msgs) if scheme != api.AUG else api.sign_batch(sg, scheme, [t['ks'][i] for i in idx], msgs)[1]
    idx[3], idx[4], msgs[6] = kc.IDENT, idx[5], b'other'
    got = api.verify_indexed_batch(ks, scheme, idx, sigs, msgs)
    assert got == api.verify_batch(sg, scheme, ks.get(idx)[0], sigs, msgs)
    assert got[:8] == [0, 0, 0, api.PK_IDENTITY, api.INVALID_SIGNATURE, 0, api.INVALID_SIGNATURE, 0] and got[8:] == [0] * (n - 8)
    idx[0], idx[1], idx[2] = kc.N, kc.BAD, 2 ** 32 - 1
    assert api.verify_indexed_batch(ks, scheme, idx, sigs, msgs)[:4] == [E_ARG, api.BAD_ENCODING, E_ARG, api.PK_IDENTITY]


@pytest.mark.parametrize('sg,scheme', COMBOS, ids=COMBO_IDS)
def test_indexed_secure(api, sets_of, sg, scheme):
    t = kc.table(api, sg)
    for legacy in ([False, True] if sg == 2 else [False]):
        sets = kc.secure_sets(api, sg, scheme, t, random.Random(11 * sg + scheme + legacy), legacy=legacy)
        bad = kc.tampered(api, sg, sets)
        ks = sets_of(sg, False)
        st = api.verify_secure_indexed_batch(ks, scheme, sets, ser_format=int(legacy))
        assert st == api.verify_secure_batch(sg, scheme, kc.gathered(api, ks, sets), ser_format=int(legacy))
        assert st == [api.OK] * len(sets)                   # the empty set's signature is the identity
        got = api.verify_secure_indexed_batch(ks, scheme, bad, ser_format=int(legacy))
        want = api.verify_secure_batch(sg, scheme, kc.gathered(api, ks, bad), ser_format=int(legacy))
        print('indexed', got, 'by value', want)
        assert got == want and len(set(want)) >= 4
        assert api.verify_secure_indexed_batch(sets_of(sg, True), scheme, sets + bad, ser_format=int(legacy)) == st + want


@pytest.mark.parametrize('sg', [1, 2])
def test_single_set_indexed(api, sets_of, sg):
    """One set alone: the by-value calls forward it to the single-set entry points, the indexed calls run it through the bodies they
    share with the by-value calls of many sets.  Five positions, one of them twice; a good signature and one over another message."""
    g = 3 - sg
    ks = sets_of(sg, False)
    want = {'good': [[api.OK]] * 2, 'tampered': [[api.INVALID_SIGNATURE]] * 2}
    got = {}
    for name, sets in single.cases(api, kc, sg, kc.multi_sets).items():
        got[name] = [api.multi_verify_indexed_batch(ks, api.BASIC, sets), api.multi_verify_batch(sg, api.BASIC, kc.gathered(api, ks, sets))]
    print('multi [indexed, by value]', got)
    assert got == want
    got = single.secure_statuses(api, kc, sg, ks)
    print('secure [indexed, by value]', got)
    assert got == want
    sums = [api.sum_indexed_batch(ks, [single.IDX]), api.sum_batch(g, [ks.get(single.IDX)[0]])]       # no signature in this one
    assert api.serialize(g, sums[0]) == api.serialize(g, sums[1]) and sums[0][0] != bytes(144 * g)


def test_single_set_indexed_large_path(api):
    """... and with BLSGPU_SECURE_BATCH_MAX=2 the lone secure set takes the one-at-a-time loop of large sets through the indexed key
    source (its by-value twin is the single call): tests/keyset_single_worker.py in a child process, as test_every_plan_same_statuses."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, BLSGPU_SECURE_BATCH_MAX='2')
    p = subprocess.run([sys.executable, os.path.join(here, 'keyset_single_worker.py')], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    print('secure [indexed, by value]', got)
    assert got == {str(sg): {'good': [[api.OK]] * 2, 'tampered': [[api.INVALID_SIGNATURE]] * 2} for sg in (1, 2)}


@pytest.mark.parametrize('tables', [False, True], ids=['ladder', 'tables'])
@pytest.mark.parametrize('sg', [1, 2])
def test_precedence(api, sets_of, sg, tables):
    """out-of-range first (in the status slot, the neighbours untouched), then the first invalid entry's creation status"""
    t, ks = kc.table(api, sg), sets_of(sg, tables)
    rng = random.Random(5 + sg)
    for call, make in ((api.multi_verify_indexed_batch, kc.multi_sets), (api.verify_secure_indexed_batch, kc.secure_sets)):
        v = make(api, sg, api.BASIC, t, rng, sizes=[3, 5, 65, 4, 6, 2, 1])
        sets = [v[0], (v[1][0] + [kc.N], v[1][1], v[1][2]), v[2], (v[3][0][:2] + [kc.BAD] + v[3][0][2:], v[3][1], v[3][2]),
                ([kc.BAD, 2 ** 32 - 1] + v[4][0], v[4][1], v[4][2]), v[5], ([2 ** 32 - 1], v[6][1], v[6][2]), v[6]]
        assert call(ks, api.BASIC, sets) == [0, E_ARG, 0, api.BAD_ENCODING, E_ARG, 0, E_ARG, 0]
    g = 3 - sg
    assert api.serialize(g, api.sum_indexed_batch(ks, [[kc.BAD], [kc.BAD, 1, kc.IDENT], []])) == \
        api.serialize(g, [kc.mb.identity(g)]) + ks.get([1], api.FMT_COMPRESSED)[0] + api.serialize(g, [kc.mb.identity(g)])
    with pytest.raises(api.BlsGpuRuntimeError):
        api.sum_indexed_batch(ks, [[1], [kc.N]])
    if sg == 2:      # the first invalid entry in input order decides
        tl = kc.table(api, 2, True)
        with api.KeySet.create(2, tl['blobs'], tl['fmt']) as kl:
            sig, msg = v[0][1], v[0][2]
            assert api.multi_verify_indexed_batch(kl, api.BASIC, [([1, kc.BAD_LEGACY, kc.BAD], sig, msg), ([kc.BAD, kc.BAD_LEGACY], sig, msg)]) == \
                [api.LEGACY_FORMAT, api.BAD_ENCODING]


def test_every_plan_same_statuses(api):
    """The strip plans, the one-at-a-time path of large secure sets and refused tables change no result: tests/keyset_worker.py in a
    child process per setting, one after another, stopping at the first that fails."""
    here = os.path.dirname(os.path.abspath(__file__))
    knobs = ('BLSGPU_MULTI_STRIP', 'BLSGPU_SECURE_BATCH_MAX', 'BLSGPU_KEYSET_TABLE_MB')
    got = {}
    for setting in ({}, {'BLSGPU_MULTI_STRIP': '1'}, {'BLSGPU_MULTI_STRIP': '3'}, {'BLSGPU_MULTI_STRIP': '64'}, {'BLSGPU_MULTI_STRIP': '4294967296'},
                    {'BLSGPU_SECURE_BATCH_MAX': '2'}, {'BLSGPU_SECURE_BATCH_MAX': '64'}, {'BLSGPU_KEYSET_TABLE_MB': '0'}):
        env = {k: x for k, x in os.environ.items() if k not in knobs}
        env.update(setting)
        p = subprocess.run([sys.executable, os.path.join(here, 'keyset_worker.py')], env=env, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (setting, p.stderr[-2000:])
        got[json.dumps(setting)] = json.loads(p.stdout.strip().splitlines()[-1])
    base = got['{}']
    assert base['1/1']['has_tables'] and base['2/1']['has_tables'] and not base['1/0']['has_tables']
    for key, r in got.items():
        for k in r:
            refused = 'TABLE_MB' in key
            assert r[k]['has_tables'] == (base[k]['has_tables'] and not refused), (key, k)
            assert {x: r[k][x] for x in ('multi', 'secure', 'sums')} == {x: base['1/0' if k[0] == '1' else '2/0'][x] for x in ('multi', 'secure', 'sums')}, (key, k)
    for sg in ('1', '2'):
        m, s = base[sg + '/0']['multi'], base[sg + '/0']['secure']
        assert m[:9] == [api.SIG_IDENTITY] + [0] * 8 and m[-2:] == [api.BAD_ENCODING, E_ARG] and len(set(m)) >= 5
        assert s[1:5] == [0] * 4 and s[-2:] == [api.INVALID_SIGNATURE, api.BAD_ENCODING]


@pytest.mark.parametrize('sg', [1, 2])
def test_device_resident_and_chained(api, sets_of, sg):
    """idx, offsets, signatures and statuses on the device (TensorOps); the signatures come straight from blsgpu_combine_shares"""
    import torch
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    t, ks = kc.table(api, sg), sets_of(sg, True)
    rng = random.Random(77 + sg)
    sets = kc.multi_sets(api, sg, api.BASIC, t, rng, sizes=[4, 65, 9])
    sets[2] = (sets[2][0] + [kc.N + 5], sets[2][1], sets[2][2])
    # every signature as a 2-of-2 sharing: the shares at x = 1, 2 of the line through (0, sig) are sig + a, sig + 2 a (a = m g)
    shares = []
    for _, sig, _ in sets:
        a1, a2 = api.sign_batch(3 - sg, api.BASIC, [5, 10], [b'', b''])[0]
        shares.append([(1, api.point_sum(sg, [sig, a1]), None), (2, api.point_sum(sg, [sig, a2]), None)])
    tens = lambda b: torch.tensor(list(b), dtype=torch.uint8, device=dev)
    i64 = lambda v: torch.tensor(list(v), dtype=torch.int64, device=dev)
    flat = [sh for st in shares for sh in st]
    sig_t, cst = ops.combine_shares(sg, tens(b''.join(int(x).to_bytes(32, 'little') for x, _, _ in flat)), tens(b''.join(p for _, p, _ in flat)), None,
                                    i64([0, 2, 4, 6]), 3)
    assert cst.cpu().tolist() == [0, 0, 0]
    allidx = [i for idx, _, _ in sets for i in idx]
    idx_t = torch.tensor([i - 2 ** 32 if i >= 2 ** 31 else i for i in allidx], dtype=torch.int32, device=dev)
    koffs = [0]
    for idx, _, _ in sets:
        koffs.append(koffs[-1] + len(idx))
    moffs, mblob = api._offsets([m for _, _, m in sets])
    st = ops.multi_verify_indexed_batch(ks, api.BASIC, idx_t, i64(koffs), sig_t, tens(mblob), i64(moffs), 3)
    assert st.device == dev and st.dtype == torch.int32 and st.cpu().tolist() == [0, 0, E_ARG]
    sums = ops.sum_indexed_batch(ks, 3 - sg, idx_t[:koffs[2]], i64(koffs[:3]), 2)
    assert api.serialize(3 - sg, [bytes(sums.cpu().tolist())[k * 144 * (3 - sg):(k + 1) * 144 * (3 - sg)] for k in range(2)]) == \
        api.serialize(3 - sg, api.sum_indexed_batch(ks, [s[0] for s in sets[:2]]))
    # a table created from device memory, entries read back on the device
    pts = tens(b''.join(kc.mb.identity(3 - sg) if s else p for p, s in zip(t['points'], t['status'])))
    torch.cuda.synchronize()
    with api.KeySet.create_device(sg, pts.data_ptr(), kc.N, api.FMT_RAW_PROJ) as kd:
        out, gst = ops.keyset_get(kd, 3 - sg, idx_t[:4], 4, api.FMT_COMPRESSED)
        assert bytes(out.cpu().tolist()) == b''.join(ks.get(allidx[:4], api.FMT_COMPRESSED)[0]) and gst.cpu().tolist() == [0] * 4
        assert ops.verify_secure_indexed_batch(kd, api.BASIC, idx_t, i64(koffs), sig_t, tens(mblob), i64(moffs), 3).cpu().tolist()[2] == E_ARG


def test_strict_env_knows_the_knob():
    """BLSGPU_STRICT_ENV=1 with BLSGPU_KEYSET_TABLE_MB set still initialises (a fresh process: the knobs are read once)"""
    env = dict(os.environ, BLSGPU_STRICT_ENV='1', BLSGPU_KEYSET_TABLE_MB='16')
    code = ('import sys; sys.path.insert(0, %r); import __graft_entry__ as ge; api = ge.import_pkg().api; api.init(); '
            'ks = api.KeySet.create(2, api.serialize(1, api.sign_batch(2, 0, [5], [b""])[0]), tables=True); print(ks.info()["has_tables"])' % util.ROOT)
    p = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == 'True', p.stderr[-2000:]
