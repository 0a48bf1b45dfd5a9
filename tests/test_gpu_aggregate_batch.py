"""Batched aggregation on the GPU: blsgpu_aggregate_secure_batch (aggregate_secure[_with_mode] for many independent sets) and
blsgpu_sum_batch (the plain sums of MultiSignature / AggregateSignature::from_signatures).  Expected points come from closed
forms computed with Python integers (tests/secure_coeffs.py), from the CPU oracle and from the single calls run on each set
alone.  Points are compared through serialize: a projective representative is not unique."""
import ctypes
import json
import os
import random
import subprocess
import sys

import pytest

import util
from aggregate_batch_cases import CLOSED_SIZES, MSG, closed_form_sets, expected_aggregates, identity, mixed_sets, signed
from multi_batch_cases import negate, valid_sets as multi_valid_sets, z_one
from secure_coeffs import R
from util import ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def ser(api, group, pts):
    return api.serialize(group, pts) if pts else []


# ------------------------------------------------------------------ 1. closed form
@pytest.mark.parametrize('sg', [1, 2])
def test_closed_form(api, sg):
    """keys k_i g, signatures k_i H(m): the aggregate is (sum_i t_i k_first(i)) H(m).  The 57-key set repeats key 10 at 40 and the
    130-key set key 3 at 129, each with a signature under another secret that the first-match rule must not use."""
    sets = closed_form_sets(api, sg, CLOSED_SIZES, random.Random(300 + sg))
    got = {}
    for legacy in ([False] if sg == 1 else [False, True]):
        pts, sts = api.aggregate_secure_batch(sg, [s[:2] for s in sets], api.LEGACY if legacy else api.MODERN)
        assert sts == [api.OK] * len(sets)
        got[legacy] = ser(api, sg, pts)
        assert got[legacy] == expected_aggregates(api, sg, sets, legacy=legacy), legacy
        assert got[legacy][0] == ser(api, sg, [identity(sg)])[0]                 # the empty set
        # had the duplicate's own signature been used, the aggregate would be another point
        for s, (pks, sigs, ks, first) in enumerate(sets):
            if first != list(range(len(pks))):
                wrong = expected_aggregates(api, sg, [(pks, sigs, ks, list(range(len(pks))))], legacy=legacy)[0]
                assert wrong != got[legacy][s]
    if sg == 2:
        assert all(a != b for a, b in zip(got[False][1:], got[True][1:]))


# ------------------------------------------------------------------ 2. oracle
@pytest.mark.parametrize('C,sg', [(ref.G1Impl, 1), (ref.G2Impl, 2)], ids=['g1', 'g2'])
def test_oracle_set_in_the_middle_of_a_batch(api, C, sg):
    rng = random.Random(90 + sg)
    pkraw, sigraw = (util.g2_raw, util.g1_raw) if sg == 1 else (util.g1_raw, util.g2_raw)
    sks = [ref.keygen_from_hash(bytes([31]) + i.to_bytes(4, 'big') + bytes(27)) for i in range(7)]
    pks = [ref.public_key(C, s) for s in sks]
    msg = b'aggregate me'
    sigs = [ref.sign(C, ref.BASIC, s, msg) for s in sks]
    pks[5], sigs[5] = pks[1], ref.sign(C, ref.BASIC, sks[1], b'another message')      # duplicate key, different signature
    others = [s[:2] for s in closed_form_sets(api, sg, [3, 20, 0, 70], random.Random(7), duplicates={})]
    mine = ([pkraw(p, rng) for p in pks], [sigraw(s, rng) for s in sigs])
    for mode in ([0] if sg == 1 else [0, 1]):
        pts, sts = api.aggregate_secure_batch(sg, others[:2] + [mine] + others[2:], mode)
        want = ref.aggregate_secure(C, pks, sigs, None if sg == 1 else mode)
        assert sts == [0] * 5 and ser(api, sg, pts)[2] == C.sig_to_bytes(want)


# ------------------------------------------------------------------ 3. equals the single call
@pytest.mark.parametrize('sg', [1, 2])
def test_equals_single_call(api, sg):
    sets = mixed_sets(api, sg, 20 + sg)
    pts, sts = api.aggregate_secure_batch(sg, sets)
    single = [api.aggregate_secure(sg, pks, sigs) for pks, sigs in sets]
    assert sts == [st for st, _ in single] == [api.OK] * len(sets)
    got, want = ser(api, sg, pts), ser(api, sg, [p for _, p in single])
    assert got == want
    ident = ser(api, sg, [identity(sg)])[0]
    assert got[3] == ident and got[9] == ident and got[0] == got[7] and len(set(got)) == len(got) - 2
    # RAW_AFFINE points in (decompressed points carry Z = 1; the identity is all-zero)
    half = {1: 96, 2: 192}

    def aff(group, raws):
        if not raws:
            return []
        zs = api.deserialize(group, api.serialize(group, raws))[0]
        return [bytes(half[group]) if r == identity(group) else p[:half[group]] for r, p in zip(raws, zs)]

    apts, asts = api.aggregate_secure_batch(sg, [(aff(3 - sg, pks), aff(sg, sigs)) for pks, sigs in sets], fmt=api.FMT_RAW_AFFINE)
    assert asts == sts and ser(api, sg, apts) == want
    # one set alone: a small one, the empty one, and one above the default plan split (which IS the single call)
    big = closed_form_sets(api, sg, [1030], random.Random(sg), duplicates={1030: (1029, 2)})[0][:2]
    for pks, sigs in (sets[2], sets[3], big):
        one = api.aggregate_secure_batch(sg, [(pks, sigs)])
        assert one[1] == [0] and ser(api, sg, one[0]) == ser(api, sg, [api.aggregate_secure(sg, pks, sigs)[1]])


# ------------------------------------------------------------------ 4. round trip on the device
@pytest.mark.parametrize('sg', [1, 2])
def test_device_round_trip_into_verify_secure_batch(api, sg):
    import torch
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    sizes = [4, 0, 1, 33, 70]
    sets = closed_form_sets(api, sg, sizes, random.Random(400 + sg), duplicates={33: (32, 0)})
    tens = lambda b: torch.tensor(list(b), dtype=torch.uint8, device=dev)
    i64 = lambda v: torch.tensor(list(v), dtype=torch.int64, device=dev)
    offs = [sum(sizes[:s]) for s in range(len(sizes) + 1)]
    pks_t = tens(b''.join(p for s in sets for p in s[0]))
    sigs_t = tens(b''.join(g for s in sets for g in s[1]))
    agg, st = ops.aggregate_secure_batch(sg, pks_t, sigs_t, i64(offs), len(sets))
    assert agg.device == dev and agg.dtype == torch.uint8 and st.device == dev and st.dtype == torch.int32
    assert st.cpu().tolist() == [0] * len(sets) and agg.numel() == len(sets) * (144 if sg == 1 else 288)
    host_pts, host_st = api.aggregate_secure_batch(sg, [s[:2] for s in sets])
    osz = 144 if sg == 1 else 288
    raw = bytes(agg.cpu().tolist())
    assert ser(api, sg, [raw[osz * s:osz * (s + 1)] for s in range(len(sets))]) == ser(api, sg, host_pts)
    # the aggregates stay where they are and verify under the same keys (the empty set: the identity signature, Ok)
    moffs, mblob = api._offsets([MSG] * len(sets))
    args = (agg, tens(mblob), i64(moffs), len(sets))
    assert ops.verify_secure_batch(sg, api.BASIC, pks_t, i64(offs), *args).cpu().tolist() == [api.OK] * len(sets)
    # one key dropped from every non-empty set
    ksz = 288 if sg == 1 else 144
    dropped = b''.join(p for s in sets for p in s[0][1:])
    doffs = [0]
    for t in sizes:
        doffs.append(doffs[-1] + max(t - 1, 0))
    got = ops.verify_secure_batch(sg, api.BASIC, tens(dropped), i64(doffs), *args).cpu().tolist()
    assert len(dropped) == ksz * doffs[-1]
    assert got == [api.OK if t == 0 else api.INVALID_SIGNATURE for t in sizes]


# ------------------------------------------------------------------ 5. every plan
def run_worker(what, env_name, value):
    env = {k: x for k, x in os.environ.items() if k != env_name}
    if value is not None:
        env[env_name] = value
    p = subprocess.run([sys.executable, os.path.join(HERE, 'aggregate_batch_worker.py'), what], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_every_plan_same_aggregates(api):
    """BLSGPU_SECURE_BATCH_MAX = 1 (every non-empty set one at a time), 8 (sets on both sides of the split), the default and 2^32
    (every set on the batched kernels) give the same points and statuses, each in a child process."""
    got = {}
    for v in ('1', '8', None, '4294967296'):          # one after another: a child that fails ends the test before the next starts
        got[v] = run_worker('secure', 'BLSGPU_SECURE_BATCH_MAX', v)
    for v, r in got.items():
        assert r == got[None], v
    for sg in (1, 2):
        sets = mixed_sets(api, sg, 70 + sg, big=40)
        assert sorted(len(p) for p, _ in sets)[1] < 8 <= max(len(p) for p, _ in sets)
        pts, sts = api.aggregate_secure_batch(sg, sets)
        assert got[None][str(sg)] == [[p.hex() for p in ser(api, sg, pts)], sts] and sts == [0] * len(sets)


# ------------------------------------------------------------------ 6. sum_batch
SUM_SIZES = [0, 1, 0, 2, 3, 63, 64, 65, 200]


@pytest.mark.parametrize('group', [1, 2])
def test_sum_batch(api, group):
    rng = random.Random(500 + group)
    sg = 3 - group                                        # the impl whose KEYS live in `group`
    ks = [rng.randrange(1, R) for _ in range(sum(SUM_SIZES))]
    pts = signed(api, sg, ks)[0]
    p1 = z_one(api, group, pts[:1])[0]
    sets, kss, at = [], [], 0
    for t in SUM_SIZES:
        sets.append(pts[at:at + t])
        kss.append(ks[at:at + t])
        at += t
    sets.append([p1, negate(group, p1)])                  # sums to the identity
    kss.append([ks[0], R - ks[0]])
    got = ser(api, group, api.sum_batch(group, sets))
    ident = ser(api, group, [identity(group)])[0]
    assert got == ser(api, group, [api.point_sum(group, s) for s in sets])
    # closed form: (sum k_i) g
    es = [sum(k) % R for k in kss]
    want = [ident] * len(sets)
    live = [i for i, e in enumerate(es) if e]
    for i, p in zip(live, ser(api, group, signed(api, sg, [es[i] for i in live])[0])):
        want[i] = p
    assert got == want and got[0] == got[2] == got[-1] == ident
    # RAW_AFFINE input
    zs = [z_one(api, group, s) if s else [] for s in sets[:-1]]
    half = 96 if group == 1 else 192
    assert ser(api, group, api.sum_batch(group, [[p[:half] for p in s] for s in zs], fmt=api.FMT_RAW_AFFINE)) == want[:-1]
    # one set is a plan with one set
    assert ser(api, group, api.sum_batch(group, [sets[-2]])) == [want[-2]] and api.sum_batch(group, []) == []


def test_sum_batch_every_strip_length(api):
    """BLSGPU_MULTI_STRIP = 1 (every addition in the fold) and 3 against the default plan, each in a child process"""
    base = run_worker('sum', 'BLSGPU_MULTI_STRIP', None)
    for v in ('1', '3'):
        assert run_worker('sum', 'BLSGPU_MULTI_STRIP', v) == base, v
    assert len(set(base['1'][0])) == 7                    # eight sets, two of them empty


@pytest.mark.parametrize('sg', [1, 2])
def test_sum_batch_output_feeds_multi_verify_batch(api, sg):
    """the summed keys as one-key sets give the verdicts of the original key sets, without leaving the device"""
    import torch
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    sizes = [3, 1, 9, 70, 5]
    v = multi_valid_sets(api, sg, api.POP, sizes, random.Random(600 + sg))
    sets = [(pks, sig, msg) for pks, sig, msg, _ in v]
    sets[1] = (sets[1][0], sets[1][1], sets[1][2] + b'!')              # wrong message
    sets[4] = (sets[4][0][:-1], sets[4][1], sets[4][2])                # a key missing
    want = api.multi_verify_batch(sg, api.POP, sets)
    assert want == [0, 1, 0, 0, 1]
    tens = lambda b: torch.tensor(list(b), dtype=torch.uint8, device=dev)
    i64 = lambda x: torch.tensor(list(x), dtype=torch.int64, device=dev)
    koffs = [0]
    for pks, _, _ in sets:
        koffs.append(koffs[-1] + len(pks))
    summed = ops.sum_batch(3 - sg, tens(b''.join(p for pks, _, _ in sets for p in pks)), i64(koffs), len(sets))
    assert summed.device == dev and summed.numel() == len(sets) * (288 if sg == 1 else 144)
    moffs, mblob = api._offsets([m for _, _, m in sets])
    st = ops.multi_verify_batch(sg, api.POP, summed, i64(range(len(sets) + 1)), tens(b''.join(s for _, s, _ in sets)), tens(mblob), i64(moffs), len(sets))
    assert st.cpu().tolist() == want


# ------------------------------------------------------------------ 7. the *_many helpers and the class constructors
def test_classes_and_many_helpers(api, pkg):
    g1, g2 = pkg.Bls12381G1Impl, pkg.Bls12381G2Impl
    B, A, P = api.BASIC, api.AUG, api.POP
    rng = random.Random(77)
    data = {}
    for impl in (g1, g2):
        sg = impl.sig_group
        ks = [rng.randrange(1, R) for _ in range(5)]
        pks, sigs = signed(api, sg, ks)
        data[sg] = (ks, [pkg.PublicKey(impl, p) for p in pks], sigs)
    S = lambda sg, scheme, i: pkg.Signature(g1 if sg == 1 else g2, scheme, data[sg][2][i])
    plain = lambda sg, idx: ser(api, sg, [signed(api, sg, [sum(data[sg][0][i] for i in idx) % R])[1][0]])[0]
    # MultiSignature / AggregateSignature.from_signatures: the sum, tagged with the first signature's scheme
    ms = pkg.MultiSignature.from_signatures([S(1, P, 0), S(1, P, 1), S(1, P, 2)])
    assert isinstance(ms, pkg.MultiSignature) and ms.scheme == P and ms.impl is g1 and ser(api, 1, [ms.raw])[0] == plain(1, [0, 1, 2])
    ag = pkg.AggregateSignature.from_signatures([S(2, A, 3), S(2, A, 4)])          # no MessageAugmentation restriction here
    assert isinstance(ag, pkg.AggregateSignature) and ag.scheme == A and ag.impl is g2 and ser(api, 2, [ag.raw])[0] == plain(2, [3, 4])
    with pytest.raises(pkg.BlsError) as e:
        pkg.MultiSignature.from_signatures([S(2, A, 3), S(2, A, 4)])
    assert e.value == pkg.BlsError('InvalidSignatureScheme')
    # mixed impls and every error case in one call
    items = [[S(1, B, 0), S(1, B, 1)], [S(2, B, 0)], [S(2, P, 0), S(2, P, 1), S(2, P, 4)], [S(1, B, 0), S(1, P, 1)], [S(2, B, 2), S(2, A, 3)],
             [S(1, A, 2), S(1, A, 3)]]
    for helper, cls in ((pkg.multi_signatures_many, pkg.MultiSignature), (pkg.aggregate_signatures_many, pkg.AggregateSignature)):
        got = helper(items)
        assert got[1] == pkg.BlsError('InvalidSignature') and got[3] == got[4] == pkg.BlsError('InvalidSignatureScheme')
        for i, (sg, idx, scheme) in {0: (1, [0, 1], B), 2: (2, [0, 1, 4], P)}.items():
            assert isinstance(got[i], cls) and got[i].scheme == scheme and got[i].impl.sig_group == sg
            assert ser(api, sg, [got[i].raw])[0] == plain(sg, idx)
        if cls is pkg.MultiSignature:
            assert got[5] == pkg.BlsError('InvalidSignatureScheme')
        else:
            assert ser(api, 1, [got[5].raw])[0] == plain(1, [2, 3]) and got[5].scheme == A
    # from_signatures_secure: equals the flat call, verifies with verify_secure, errors as the reference
    for sg, impl in ((1, g1), (2, g2)):
        ks, keys, sigs = data[sg]
        sgs = [S(sg, P, i) for i in range(5)]
        agg = pkg.AggregateSignature.from_signatures_secure(sgs, keys)
        assert isinstance(agg, pkg.AggregateSignature) and agg.scheme == P and agg.impl is impl
        assert ser(api, sg, [agg.raw]) == ser(api, sg, [api.aggregate_secure(sg, [k.raw for k in keys], sigs)[1]])
        assert api.verify_secure(sg, api.BASIC, [k.raw for k in keys], agg.raw, MSG) == api.OK
    with pytest.raises(pkg.BlsError) as e:
        pkg.AggregateSignature.from_signatures_secure([S(1, B, 0)], data[1][1][:2])
    assert e.value == pkg.BlsError('InvalidInputs', 'Mismatched array lengths')
    many = pkg.aggregate_secure_many([([S(1, B, i) for i in range(5)], data[1][1]), ([], []), ([S(2, B, i) for i in range(3)], data[2][1][:3]),
                                      ([S(2, B, 0), S(2, P, 1)], data[2][1][:2]), ([S(2, B, i) for i in range(3)], data[2][1][:3], api.LEGACY),
                                      ([S(2, B, 0)], [])])
    assert many[1] == pkg.BlsError('InvalidInputs', 'Empty signatures array') and many[3] == pkg.BlsError('InvalidSignatureScheme')
    assert many[5] == pkg.BlsError('InvalidInputs', 'Mismatched array lengths')
    for i, (sg, n, mode) in {0: (1, 5, api.MODERN), 2: (2, 3, api.MODERN), 4: (2, 3, api.LEGACY)}.items():
        want = api.aggregate_secure(sg, [k.raw for k in data[sg][1][:n]], data[sg][2][:n], mode)[1]
        assert isinstance(many[i], pkg.AggregateSignature) and many[i].scheme == B and ser(api, sg, [many[i].raw]) == ser(api, sg, [want])
    assert many[2].raw != many[4].raw


# ------------------------------------------------------------------ 8. argument checks
def test_argument_checks(api):
    lib = api.init()
    E_ARG = -3
    pks, sigs = signed(api, 2, [3, 5, 7, 11, 13])
    pkb, sgb = b''.join(pks), b''.join(sigs)
    out = ctypes.create_string_buffer(288 * 2)
    st = (ctypes.c_int32 * 2)(-99, -99)
    vp = lambda x: ctypes.cast(x, ctypes.c_void_p)

    def agg(sg, koffs, n_sets=2, ser_format=0, fmt=0, pk=pkb, sig=sgb, o=out, s=st):
        ko = (ctypes.c_uint64 * len(koffs))(*koffs) if koffs is not None else None
        return lib.blsgpu_aggregate_secure_batch(sg, api._ptr(pk) if pk else None, api._ptr(sig) if sig else None, vp(ko) if ko is not None else None,
                                                 n_sets, ser_format, fmt, vp(o) if o is not None else None, vp(s) if s is not None else None)

    assert agg(2, [0, 2, 5]) == 0 and list(st) == [0, 0]
    want = [api.aggregate_secure(2, pks[a:b], sigs[a:b])[1] for a, b in ((0, 2), (2, 5))]
    assert api.serialize(2, [out.raw[:288], out.raw[288:]]) == api.serialize(2, want)
    assert agg(2, [0, 3, 2]) == E_ARG                      # decreasing
    assert agg(2, [1, 2, 5]) == E_ARG                      # first offset not 0
    assert agg(2, [0, 2, 2 ** 32]) == E_ARG                # 2^32 keys
    assert agg(1, [0, 2, 5], ser_format=1) == E_ARG        # Legacy with Bls12381G1Impl
    assert agg(2, [0, 2, 5], ser_format=2) == E_ARG
    assert agg(2, [0, 2, 5], fmt=api.FMT_COMPRESSED) == E_ARG
    assert agg(3, [0, 2, 5]) == E_ARG
    assert agg(2, None) == E_ARG and agg(2, [0, 2, 5], pk=None) == E_ARG and agg(2, [0, 2, 5], sig=None) == E_ARG
    assert agg(2, [0, 2, 5], o=None) == E_ARG and agg(2, [0, 2, 5], s=None) == E_ARG
    assert agg(2, [0], n_sets=0) == 0 and agg(2, [0], n_sets=0, pk=None, sig=None, o=None, s=None) == 0
    assert agg(2, [0, 0, 0], pk=None, sig=None) == 0 and list(st) == [0, 0]      # only empty sets: no points needed

    def total(group, offs, n_sets=2, fmt=0, p=pkb, o=out):
        oo = (ctypes.c_uint64 * len(offs))(*offs) if offs is not None else None
        return lib.blsgpu_sum_batch(group, api._ptr(p) if p else None, vp(oo) if oo is not None else None, n_sets, fmt, vp(o) if o is not None else None)

    assert total(1, [0, 2, 5]) == 0
    assert api.serialize(1, [out.raw[:144], out.raw[144:288]]) == api.serialize(1, [api.point_sum(1, pks[:2]), api.point_sum(1, pks[2:])])
    assert total(1, [0, 3, 2]) == E_ARG and total(1, [1, 2, 5]) == E_ARG and total(1, [0, 2, 2 ** 32]) == E_ARG
    assert total(1, [0, 2, 5], fmt=api.FMT_COMPRESSED) == E_ARG and total(0, [0, 2, 5]) == E_ARG and total(3, [0, 2, 5]) == E_ARG
    assert total(1, None) == E_ARG and total(1, [0, 2, 5], p=None) == E_ARG and total(1, [0, 2, 5], o=None) == E_ARG
    assert total(1, [0], n_sets=0) == 0 and total(1, [0], n_sets=0, p=None, o=None) == 0
    assert total(1, [0, 0, 0], p=None) == 0 and out.raw[:288] == bytes(288)
