"""Threshold signcryption on the GPU (blsgpu_signcrypt_share_verify_batch, blsgpu_signcrypt_open_batch): the case list of
tests/signcrypt_cases.py through the flat calls and TensorOps, against hand-built two-pair checks and combine_shares + serialize,
RAW_AFFINE input, the edge shapes, and the reference's sign_crypt_with_shares_works through the wrapper types."""
import ctypes
import random

import pytest

import signcrypt_cases as sc
import util
from util import ref

pytestmark = pytest.mark.gpu
R = sc.R


def by_scheme(sg):
    out = {}
    for cs in sc.cases(sg):
        out.setdefault(cs.scheme, []).append(cs)
    return out


def share_pts(cs, rng=None):
    return [(sc.raw_pk(cs.sg, sc.pk_point(cs.sg, a), rng), sc.raw_pk(cs.sg, sc.pk_point(cs.sg, b), rng)) for _, a, b in cs.shares]


def open_shares(cs, rng=None):
    return [(i, sc.raw_pk(cs.sg, sc.pk_point(cs.sg, a), rng)) for i, a, _ in cs.shares]


@pytest.mark.parametrize('sg', [1, 2])
def test_case_list_flat_calls(api, sg):
    """One call per (impl, scheme) and entry point; points under random Z."""
    rng = random.Random(sg)
    for scheme, cl in sorted(by_scheme(sg).items()):
        cts = [sc.raw_ct(cs, rng) for cs in cl]
        got = api.signcrypt_share_verify_batch(sg, scheme, cts, [share_pts(cs, rng) for cs in cl])
        assert got == [cs.share_statuses() for cs in cl], scheme
        plain, st = api.signcrypt_open_batch(sg, scheme, cts, [open_shares(cs, rng) for cs in cl], with_status=True)
        want = [cs.open_with_shares() for cs in cl]
        assert st == [w[0] for w in want], [(cs.name, s, w[0]) for cs, s, w in zip(cl, st, want) if s != w[0]]
        assert plain == [w[1] for w in want]
        plain, st = api.signcrypt_decrypt_batch(sg, scheme, cts, [sc.raw_pk(sg, sc.pk_point(sg, cs.key), rng) for cs in cl], with_status=True)
        want = [cs.open_with_key() for cs in cl]
        assert (st, plain) == ([w[0] for w in want], [w[1] for w in want])


def affine(sg, group_is_pk, raw):
    """RAW_PROJ with Z = 1 (or the identity) -> RAW_AFFINE."""
    g2 = (sg == 1) == group_is_pk
    half = 192 if g2 else 96
    ident = (util.g2_raw if g2 else util.g1_raw)(None)
    return bytes(half) if raw == ident else raw[:half]


@pytest.mark.parametrize('sg', [1, 2])
def test_affine_input_gives_the_same(api, sg):
    cl = by_scheme(sg)[ref.BASIC]
    cts = [sc.raw_ct(cs) for cs in cl]
    acts = [(affine(sg, True, u), v, affine(sg, False, w)) for u, v, w in cts]
    sh = [[(affine(sg, True, a), affine(sg, True, b)) for a, b in share_pts(cs)] for cs in cl]
    assert api.signcrypt_share_verify_batch(sg, ref.BASIC, acts, sh, fmt=api.FMT_RAW_AFFINE) == [cs.share_statuses() for cs in cl]
    osh = [[(i, affine(sg, True, p)) for i, p in open_shares(cs)] for cs in cl]
    want = [cs.open_with_shares() for cs in cl]
    plain, st = api.signcrypt_open_batch(sg, ref.BASIC, acts, osh, fmt=api.FMT_RAW_AFFINE, with_status=True)
    assert (st, plain) == ([w[0] for w in want], [w[1] for w in want])


@pytest.mark.parametrize('sg', [1, 2])
def test_tensor_ops_device_resident(api, sg):
    import torch
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    cl = by_scheme(sg)[ref.BASIC]
    cts = [sc.raw_ct(cs) for cs in cl]
    n_ct = len(cl)
    tens = lambda b: torch.tensor(list(b), dtype=torch.uint8, device=dev)
    i64 = lambda xs: torch.tensor(xs, dtype=torch.int64, device=dev)
    us, ws, vs = tens(b''.join(u for u, _, _ in cts)), tens(b''.join(w for _, _, w in cts)), tens(b''.join(v for _, v, _ in cts) or b'\0')
    voffs = [0]
    for _, v, _ in cts:
        voffs.append(voffs[-1] + len(v))
    soffs = [0]
    for cs in cl:
        soffs.append(soffs[-1] + len(cs.shares))
    sh = [p for cs in cl for p in share_pts(cs)]
    shares_t, pks_t = tens(b''.join(a for a, _ in sh)), tens(b''.join(b for _, b in sh))
    ids_t = tens(b''.join(int(i).to_bytes(32, 'little') for cs in cl for i, _, _ in cs.shares))
    st = ops.signcrypt_share_verify_batch(sg, ref.BASIC, us, ws, vs, i64(voffs), n_ct, shares_t, pks_t, i64(soffs), len(sh))
    assert st.is_cuda and st.cpu().tolist() == [s for cs in cl for s in cs.share_statuses()]
    frames, rng_t, st = ops.signcrypt_open_batch(sg, ref.BASIC, us, ws, vs, i64(voffs), n_ct, ids_t, shares_t, i64(soffs))
    assert frames.is_cuda and rng_t.is_cuda and st.is_cuda
    fr, rg = bytes(frames.cpu().tolist()), rng_t.cpu().tolist()
    want = [cs.open_with_shares() for cs in cl]
    assert st.cpu().tolist() == [w[0] for w in want]
    for c, w in enumerate(want):
        if w[0] == sc.OK:
            assert fr[voffs[c] + rg[c][0]:voffs[c] + rg[c][0] + rg[c][1]] == w[1], cl[c].name
        else:
            assert rg[c] == [0, 0]
    keys_t = tens(b''.join(sc.raw_pk(sg, sc.pk_point(sg, cs.key)) for cs in cl))
    _, _, st = ops.signcrypt_decrypt_batch(sg, ref.BASIC, us, ws, vs, i64(voffs), n_ct, keys_t)
    assert st.cpu().tolist() == [cs.open_with_key()[0] for cs in cl]


@pytest.mark.parametrize('sg', [1, 2])
def test_share_verdicts_equal_hand_built_pairs(api, sg):
    """(-W', share) (w, pk) through pairing2_check_batch, W' from hash_to_point: the same verdicts where no identity is involved."""
    import multi_batch_cases as mbc
    C = sc.IMPLS[sg]
    cl = [cs for cs in by_scheme(sg)[ref.BASIC] if cs.shares and cs.w is not None]
    hashes = api.hash_to_point(sg, [cs.hashed() for cs in cl], C.DST[ref.BASIC])
    a1, a2, b1, b2, want = [], [], [], [], []
    for cs, h in zip(cl, hashes):
        for (sh, pk), (_, a, b) in zip(share_pts(cs), cs.shares):
            if a % R == 0 or b % R == 0:
                continue
            nh, w = mbc.negate(sg, h), sc.raw_sig(sg, cs.w)
            g1a, g2a, g1b, g2b = (nh, sh, w, pk) if sg == 1 else (sh, nh, pk, w)
            a1.append(g1a), a2.append(g2a), b1.append(g1b), b2.append(g2b)
            want.append(cs.share_status(a, b) == sc.OK)
    assert len(want) > 20 and True in want and False in want
    assert api.pairing2_check_batch(a1, a2, b1, b2) == want


@pytest.mark.parametrize('sg', [1, 2])
def test_recovered_keys_equal_combine_and_serialize(api, sg):
    """Opening with the key that combine_shares recovers gives the frames the share form gives; the key bytes are the model's."""
    cl = [cs for cs in by_scheme(sg)[ref.BASIC] if len(cs.shares) >= 2]
    g = 3 - sg
    keys, _ = api.combine_shares(g, [[(i, p, None) for i, p in open_shares(cs)] for cs in cl])
    C = sc.IMPLS[sg]
    want = [C.pk_to_bytes(sc.pk_point(sg, sc.combined_scalar([(i, a) for i, a, _ in cs.shares]))) for cs in cl]
    assert api.serialize(g, keys) == want
    cts = [sc.raw_ct(cs) for cs in cl]
    assert api.signcrypt_decrypt_batch(sg, ref.BASIC, cts, keys, with_status=True) == \
        api.signcrypt_open_batch(sg, ref.BASIC, cts, [open_shares(cs) for cs in cl], with_status=True)


def device_points(api, sg, ks):
    return api.sign_batch(sg, api.BASIC, [k % R for k in ks], [b''] * len(ks))[0]


@pytest.mark.parametrize('sg', [1, 2])
def test_edge_shapes(api, sg):
    assert api.signcrypt_share_verify_batch(sg, ref.BASIC, [], []) == []
    assert api.signcrypt_open_batch(sg, ref.BASIC, [], [], with_status=True) == ([], [])
    base = sc.cases(sg)[0]
    cts = [sc.raw_ct(base)] * 3
    assert api.signcrypt_share_verify_batch(sg, ref.BASIC, cts, [[], [], []]) == [[], [], []]
    assert api.signcrypt_open_batch(sg, ref.BASIC, cts, [[], [], []], with_status=True) == ([None] * 3, [sc.VSSS_ERROR] * 3)
    # 65 ciphertexts x 2 shares: more than one workgroup of ciphertexts, 130 shares; every third share pair is swapped
    p = [sc._scalar(b'edge', sg), sc._scalar(b'edgeb', sg)]
    cl = [sc.sealed(sg, 'edge %d' % k, ref.BASIC, b'message %d' % k * (k % 5), p, [1 + k, 70 + k]) for k in range(65)]
    flat = [x for cs in cl for _, a, b in cs.shares for x in (a, b)]
    pts = device_points(api, sg, flat)
    sh = [[(pts[4 * k], pts[4 * k + 1]), (pts[4 * k + 2], pts[4 * k + 3])] for k in range(65)]
    want = [[sc.OK, sc.OK] for _ in cl]
    for k in range(0, 65, 3):
        sh[k][1] = (sh[k][0][0], sh[k][1][1])
        want[k][1] = sc.INVALID_DECRYPTION_SHARE
    cts = [sc.raw_ct(cs) for cs in cl]
    assert api.signcrypt_share_verify_batch(sg, ref.BASIC, cts, sh) == want
    osh = [[(cs.shares[0][0], pts[4 * k]), (cs.shares[1][0], pts[4 * k + 2])] for k, cs in enumerate(cl)]
    assert api.signcrypt_open_batch(sg, ref.BASIC, cts, osh) == [cs.message for cs in cl]


@pytest.mark.parametrize('sg', [1, 2])
def test_one_ciphertext_1100_shares(api, sg):
    """Above the default BLSGPU_SHARES_MSM_MIN: the share sum takes the MSM plan."""
    rng = random.Random(1100 + sg)
    coeffs = [rng.randrange(1, R) for _ in range(5)]
    ids = rng.sample(range(1, 10 ** 9), 1100)
    cs = sc.sealed(sg, '1100 shares', ref.BASIC, b'opened by eleven hundred shares', coeffs, ids)
    pts = device_points(api, sg, [a for _, a, _ in cs.shares])
    plain, st = api.signcrypt_open_batch(sg, ref.BASIC, [sc.raw_ct(cs)], [[(i, p) for (i, _, _), p in zip(cs.shares, pts)]], with_status=True)
    assert (st, plain) == ([sc.OK], [cs.message])


@pytest.mark.parametrize('sg', [1, 2])
def test_wrapper_types_sign_crypt_with_shares_works(api, sg):
    """reference tests/encryption.rs:37-61."""
    impl = api.Bls12381G1Impl if sg == 1 else api.Bls12381G2Impl
    msg = b'Hello World!'
    p = [sc._scalar(b'wrap', sg), sc._scalar(b'wrapb', sg)]
    cs = sc.sealed(sg, 'wrapper', ref.BASIC, msg, p, [1, 2, 3])
    u, v, w = sc.raw_ct(cs)
    ct = api.SignCryptCiphertext(impl, api.BASIC, u, v, w)
    assert ct.is_valid()
    sp = share_pts(cs)
    shares = [api.SignDecryptionShare(impl, i, a) for (i, _, _), (a, _) in zip(cs.shares, sp)]
    pks = [api.PublicKeyShare(impl, i, b) for (i, _, _), (_, b) in zip(cs.shares, sp)]
    for s, k in zip(shares, pks):
        s.verify(k, ct)
    with pytest.raises(api.BlsError) as e:
        shares[0].verify(pks[1], ct)
    assert e.value.kind == 'InvalidDecryptionShare'
    assert ct.decrypt_with_shares(shares) == msg
    assert ct.decrypt_with_shares(shares[:2]) == msg
    assert ct.decrypt_with_shares(shares[2:]) is None
    key = api.SignCryptDecryptionKey.from_shares(shares)
    assert key.decrypt(ct) == msg
    with pytest.raises(api.BlsError) as e:
        api.SignCryptDecryptionKey.from_shares(shares[:1])
    assert e.value.kind == 'VsssError'
    other = sc.cases(sg)[1]                                  # an Aug ciphertext in the same call group-by
    ct2 = api.SignCryptCiphertext(impl, other.scheme, *sc.raw_ct(other))
    sh2 = [api.SignDecryptionShare(impl, i, q) for i, q in open_shares(other)]
    assert api.open_many([(ct, shares), (ct2, sh2), (ct, shares[2:])]) == [msg, other.message, None]


@pytest.mark.parametrize('sg', [1, 2])
def test_basic_dst_quirk(api, sg):
    """SignDecryptionShare::verify passes the Basic DST whatever the ciphertext's scheme is (src/sign_decryption_share.rs:54): an
    honest share of an Aug ciphertext is rejected by the wrapper type and accepted by the flat call with scheme = AUG."""
    impl = api.Bls12381G1Impl if sg == 1 else api.Bls12381G2Impl
    cs = sc.cases(sg)[1]
    assert cs.scheme == ref.AUG
    u, v, w = sc.raw_ct(cs)
    (a, b) = share_pts(cs)[0]
    assert api.signcrypt_share_verify_batch(sg, api.AUG, [(u, v, w)], [[(a, b)]]) == [[sc.OK]]
    assert api.signcrypt_share_verify_batch(sg, api.BASIC, [(u, v, w)], [[(a, b)]]) == [[sc.INVALID_DECRYPTION_SHARE]]
    with pytest.raises(api.BlsError) as e:
        api.SignDecryptionShare(impl, cs.shares[0][0], a).verify(api.PublicKeyShare(impl, cs.shares[0][0], b), api.SignCryptCiphertext(impl, api.AUG, u, v, w))
    assert e.value.kind == 'InvalidDecryptionShare'


def test_bad_offsets_are_argument_errors(api):
    lib = api.init()
    cs = sc.cases(2)[0]
    u, v, w = sc.raw_ct(cs)
    (a, b) = share_pts(cs)[0]
    st = (ctypes.c_int32 * 4)()
    rng = (ctypes.c_uint64 * 4)()
    frames = ctypes.create_string_buffer(len(v))
    ids = (1).to_bytes(32, 'little')
    off = lambda *xs: ctypes.cast((ctypes.c_uint64 * len(xs))(*xs), ctypes.c_void_p)
    p = api._ptr
    for voffs, soffs in (((0, len(v)), (1, 1)), ((0, len(v)), (0, 2 ** 33)), ((1, len(v)), (0, 1)), ((0, len(v), 3)[:2], (1, 0))):
        assert lib.blsgpu_signcrypt_share_verify_batch(2, 0, p(u), p(w), p(v), off(*voffs), 1, p(a), p(b), off(*soffs), 0, ctypes.cast(st, ctypes.c_void_p)) == -3
    assert lib.blsgpu_signcrypt_share_verify_batch(2, 0, p(u), p(w), p(v), off(0, len(v), 5), 2, p(a), p(b), off(0, 1, 0), 0, ctypes.cast(st, ctypes.c_void_p)) == -3
    assert lib.blsgpu_signcrypt_open_batch(2, 0, p(u), p(w), p(v), off(0, len(v)), 1, p(ids), p(a), off(2, 3), 0, ctypes.cast(frames, ctypes.c_void_p),
                                           ctypes.cast(rng, ctypes.c_void_p), ctypes.cast(st, ctypes.c_void_p)) == -3
    assert lib.blsgpu_signcrypt_open_batch(2, 0, p(u), p(w), p(v), off(0, len(v)), 1, p(ids), p(a), None, 0, ctypes.cast(frames, ctypes.c_void_p),
                                           ctypes.cast(rng, ctypes.c_void_p), ctypes.cast(st, ctypes.c_void_p)) == -3
    assert lib.blsgpu_signcrypt_open_batch(2, 0, p(u), p(w), p(v), off(0, len(v)), 1, None, p(a), None, 3, ctypes.cast(frames, ctypes.c_void_p),
                                           ctypes.cast(rng, ctypes.c_void_p), ctypes.cast(st, ctypes.c_void_p)) == -3
