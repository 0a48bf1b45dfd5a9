"""Timestamp proofs of knowledge on the device: blsgpu_hash_to_scalar, blsgpu_sig_proof_challenge_batch and
blsgpu_sig_proof_timestamp_verify_batch against the CPU restatement of tests/pok_timestamp_cases.py (never against another GPU
call, except where the test says that two calls must agree).  Sizes: 1, 63, 64, 65, 130 around the 64-lane workgroup; 513 and 4,097
just past BLSGPU_WIDE_MAX (512) and BLSGPU_COOP_MAX (4,096), where run_pairing2 changes plan."""
import random

import pytest

import pok_timestamp_cases as pc
from oracle.py import bls381 as c

pytestmark = pytest.mark.gpu

SKIPPED_KERNELS = ('k_wide', 'k_pairing_coop', 'k_lines2s', 'k_millerf2s', 'k_finalexp2s', 'k_miller2s', 'k_finalexps', 'k_cyc_run4',
                   'k_pairing_coop_keyed', 'k_prepare', 'k_proof_challenge')


def T(torch, dev, b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) if b else torch.zeros(0, dtype=torch.uint8, device=dev)


def I64(torch, dev, xs):
    """u64 values as the bits of an int64 tensor"""
    return torch.tensor([x - (1 << 64) if x >> 63 else x for x in xs], dtype=torch.int64, device=dev)


# ------------------------------------------------------------------ hash_to_scalar
@pytest.mark.parametrize('salt', sorted(pc.SALTS))
@pytest.mark.parametrize('n', pc.SIZES)
def test_hash_to_scalar(api, n, salt):
    msgs = pc.hash_inputs(n, 100 * n + len(salt))
    if n >= 63:
        msgs[0], msgs[1], msgs[n - 1] = b'', msgs[1][:1] or b'x', (msgs[n - 1] * 200 + b'z' * 200)[:200]
    got = api.hash_to_scalar(msgs, pc.SALTS[salt])
    assert got == [pc.hash_to_scalar(m, pc.SALTS[salt]) for m in msgs]


def test_hash_to_scalar_every_length_and_empty_salt(api):
    msgs = [bytes((7 * i + j) & 255 for j in range(i)) for i in pc.MSG_LENS]
    for salt in (b'', pc.POK_SALT):
        assert api.hash_to_scalar(msgs, salt) == [pc.hash_to_scalar(m, salt) for m in msgs]
    assert api.hash_to_scalar([], pc.POK_SALT) == []


def test_hash_to_scalar_on_device(api):
    import torch
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    msgs = pc.hash_inputs(65, 7)
    offs = [0]
    for m in msgs:
        offs.append(offs[-1] + len(m))
    salt = pc.SALTS['long65']
    out = ops.hash_to_scalar(T(torch, dev, b''.join(msgs)), torch.tensor(offs, dtype=torch.int64, device=dev), 65, T(torch, dev, salt), len(salt))
    raw = bytes(out.cpu().tolist())
    assert [int.from_bytes(raw[32 * i:32 * i + 32], 'little') for i in range(65)] == [pc.hash_to_scalar(m, salt) for m in msgs]


# ------------------------------------------------------------------ sig_proof_challenge_batch
@pytest.mark.parametrize('fmt', (pc.RAW_PROJ, pc.RAW_AFFINE, pc.COMPRESSED, pc.LEGACY))
@pytest.mark.parametrize('n', pc.SIZES)
@pytest.mark.parametrize('sg', (1, 2))
def test_challenge_batch(api, sg, n, fmt):
    C = pc.IMPLS[sg]
    rng = random.Random(1000 * sg + 10 * n + fmt)
    pts = pc.points(sg)
    us = [pts[(i + n) % len(pts)] for i in range(n)]          # the identity among them
    ts = [(0, 1, 1 << 32, pc.U64_MAX, pc.NOW)[i % 5] if i < 10 else rng.getrandbits(64) for i in range(n)]
    got = api.sig_proof_challenge_batch(sg, [pc.render_point(sg, u, fmt, rng) for u in us], ts, fmt=fmt)     # a fresh Z per occurrence
    assert got == [pc.compute_y(C, u, t) for u, t in zip(us, ts)]


def test_challenge_batch_bad_encoding_and_device(api):
    import torch
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    for sg in (1, 2):
        C = pc.IMPLS[sg]
        rng = random.Random(sg)
        us = list(pc.points(sg)) * 11                        # 66 items
        ts = [rng.getrandbits(64) for _ in us]
        want = [pc.compute_y(C, u, t) for u, t in zip(us, ts)]
        out = ops.sig_proof_challenge_batch(sg, T(torch, dev, b''.join(pc.render_point(sg, u, pc.RAW_PROJ, rng) for u in us)), I64(torch, dev, ts), len(us))
        raw = bytes(out.cpu().tolist())
        assert [int.from_bytes(raw[32 * i:32 * i + 32], 'little') for i in range(len(us))] == want
        # x = p is not a field element: the commitment does not decode, its challenge is zero; its neighbours are untouched
        wire = [pc.render_point(sg, u, pc.COMPRESSED, rng) for u in us]
        bad = bytearray(48 * sg)
        bad[-48:] = c.P.to_bytes(48, 'big')
        bad[0] |= 0x80
        wire[3] = bytes(bad)
        got = api.sig_proof_challenge_batch(sg, wire, ts, fmt=pc.COMPRESSED)
        assert got[3] == 0 and got[:3] == want[:3] and got[4:] == want[4:]
    assert api.sig_proof_challenge_batch(1, [], []) == []


# ------------------------------------------------------------------ sig_proof_timestamp_verify_batch
def run_verify(api, sg, scheme, n, mode, fmt=pc.RAW_PROJ, seed=0, kinds=pc.KINDS):
    (us, vs, pks, ts, msgs), want, names = pc.build_batch(sg, scheme, n, mode, fmt=fmt, seed=seed, kinds=kinds)
    got = api.sig_proof_timestamp_verify_batch(sg, scheme, us, vs, pks, ts, msgs, pc.NOW, pc.MODES[mode], fmt=fmt)
    assert got == want, [(i, nm, g, w) for i, (nm, g, w) in enumerate(zip(names, got, want)) if g != w][:10]
    return (us, vs, pks, ts, msgs), want, names


@pytest.mark.parametrize('mode', sorted(pc.MODES))
@pytest.mark.parametrize('scheme', pc.SCHEMES)
@pytest.mark.parametrize('sg', (1, 2))
def test_verify_every_kind(api, sg, scheme, mode):
    (us, vs, pks, ts, msgs), want, names = run_verify(api, sg, scheme, 65, mode)
    assert set(names) == set(pc.KINDS)
    # the same statuses as the two-call form wherever no timeout rule applies
    ys = api.sig_proof_challenge_batch(sg, us, ts)
    two = api.sig_proof_verify_batch(sg, scheme, us, vs, pks, ys, msgs)
    for i, nm in enumerate(names):
        if mode == 'none' or nm not in pc.TIMEOUT_RULED:
            assert two[i] == want[i], (i, nm)


@pytest.mark.parametrize('n', (513, 4097))
@pytest.mark.parametrize('scheme', pc.SCHEMES)
@pytest.mark.parametrize('sg', (1, 2))
def test_verify_past_the_plan_changes(api, sg, scheme, n):
    run_verify(api, sg, scheme, n, 'timeout', seed=n)


@pytest.mark.parametrize('fmt', (pc.RAW_AFFINE, pc.COMPRESSED, pc.LEGACY))
@pytest.mark.parametrize('sg', (1, 2))
def test_verify_other_formats(api, sg, fmt):
    from oracle.py import blsful_ref as ref
    (us, vs, pks, ts, msgs), want, names = run_verify(api, sg, ref.POP, 65, 'timeout', fmt=fmt, seed=fmt)
    if fmt == pc.RAW_AFFINE:
        return
    # a commitment, a proof and a key that do not decode: the decode status of the first of them, unless the timeout rule speaks
    def bad(width):
        b = bytearray(width)
        b[-48:] = c.P.to_bytes(48, 'big')
        b[0] |= 0x80
        if fmt == pc.LEGACY:
            b = bytearray(ref.modern_to_legacy(bytes(b)))
        return bytes(b)
    us, vs, pks = list(us), list(vs), list(pks)
    v0, l0 = names.index('valid'), names.index('past_limit')
    us[v0] = bad(48 * sg)
    vs[v0 + len(pc.KINDS)] = bad(48 * sg)
    pks[v0 + 2 * len(pc.KINDS)] = bad(48 * (3 - sg))
    us[l0] = bad(48 * sg)
    got = api.sig_proof_timestamp_verify_batch(sg, ref.POP, us, vs, pks, ts, msgs, pc.NOW, pc.TIMEOUT, fmt=fmt)
    for k in range(3):
        assert got[v0 + k * len(pc.KINDS)] == api.BAD_ENCODING, (k, got[v0 + k * len(pc.KINDS)])
        want[v0 + k * len(pc.KINDS)] = api.BAD_ENCODING
    assert got == want and got[l0] == pc.INVALID_SIGNATURE


def test_verify_on_device(api):
    import torch
    from oracle.py import blsful_ref as ref
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    for sg in (1, 2):
        (us, vs, pks, ts, msgs), want, _ = pc.build_batch(sg, ref.AUG, 65, 'timeout', seed=3)
        offs = [0]
        for m in msgs:
            offs.append(offs[-1] + len(m))
        st = ops.sig_proof_timestamp_verify_batch(sg, ref.AUG, T(torch, dev, b''.join(us)), T(torch, dev, b''.join(vs)), T(torch, dev, b''.join(pks)),
                                                  I64(torch, dev, ts), T(torch, dev, b''.join(msgs)), torch.tensor(offs, dtype=torch.int64, device=dev), 65,
                                                  pc.NOW, pc.TIMEOUT)
        assert st.device.type == 'cuda' and st.cpu().tolist() == want


def test_timed_out_items_skip_the_pairing(api):
    from oracle.py import blsful_ref as ref
    late = ('past_limit', 'past_limit_u_inf', 't_zero')
    api.profile_enable(True)
    try:
        before = {k: v[1] for k, v in api.profile_read().items()}
        for sg, n in ((1, 65), (2, 513)):
            _, want, _ = run_verify(api, sg, ref.BASIC, n, 'timeout', kinds=late)
            assert want == [pc.INVALID_SIGNATURE] * n
        now = {k: v[1] for k, v in api.profile_read().items()}
    finally:
        api.profile_enable(False)
    assert now.get('k_proof_timeout', 0) - before.get('k_proof_timeout', 0) == 2
    for k in SKIPPED_KERNELS:
        assert now.get(k, 0) == before.get(k, 0), k


def test_classes_and_many(api, pkg):
    from oracle.py import blsful_ref as ref
    sg, scheme = 2, ref.POP
    impl = pkg.Bls12381G2Impl
    its = pc.items(sg, scheme)
    rng = random.Random(5)

    def mk(kind):
        u, v, pk, t, msg = its[kind]
        return (pkg.ProofOfKnowledgeTimestamp(impl, scheme, pc.render_point(sg, u, 0, rng), pc.render_point(sg, v, 0, rng), t),
                pkg.PublicKey(impl, pc.render_point(3 - sg, pk, 0, rng)), msg)
    kinds = ('valid', 'past_limit', 'future_with_timeout', 'u_inf', 'msg_flip')
    errs = api.proof_timestamp_verify_many([mk(k) for k in kinds], pc.NOW, pc.TIMEOUT)
    assert errs[0] is None and errs[1] == pkg.BlsError('InvalidProof') and isinstance(errs[2], api.BlsGpuRuntimeError)
    assert errs[3] == pkg.BlsError('InvalidInputs', 'commitment is the identity point') and errs[4] == pkg.BlsError('InvalidProof')
    pr, pk, msg = mk('valid')
    pr.verify(pk, msg, timeout_ms=pc.TIMEOUT, now_ms=pc.NOW)
    pr.verify(pk, msg)                                           # no timeout: this host's clock plays no part
    with pytest.raises(pkg.BlsError):
        pr.verify(pk, msg, timeout_ms=1)                         # the host's clock: NOW - 1000 is long past
    u, v, _, t, _ = its['valid']
    y = pc.compute_y(pc.IMPLS[sg], u, t)
    pkg.ProofOfKnowledge(impl, scheme, pr.u, pr.v).verify(pk, msg, y)
    with pytest.raises(pkg.BlsError):
        pkg.ProofOfKnowledge(impl, scheme, pr.u, pr.v).verify(pk, msg, y + 1)
    ch = pkg.ProofCommitmentChallenge.from_hash(impl, b'challenge seed')
    assert ch.value == pc.hash_to_scalar(b'challenge seed', pc.KEYGEN_SALT)
    assert ch.to_le_bytes() == ch.value.to_bytes(32, 'little') and ch.to_be_bytes() == ch.to_le_bytes()[::-1]
