"""ElGamal on the GPU (blsgpu_elgamal_message_generator, blsgpu_elgamal_proof_verify_batch, blsgpu_elgamal_open_batch): the case
list of tests/elgamal_cases.py through the flat call and TensorOps against the Python restatement of the reference, the edge
shapes, every input format, the opening against combine_shares plus a subtraction in the oracle, and the reference's
elgamal_ciphertext_works through the wrapper types."""
import ctypes
import random

import pytest

import elgamal_cases as ec
from util import c

pytestmark = pytest.mark.gpu
R = c.R


def names(cl, got):
    return [(cs.name, g, cs.expect) for cs, g in zip(cl, got) if g != cs.expect]


@pytest.mark.parametrize('sg', [1, 2])
def test_message_generator(api, sg):
    g = ec.kg(sg)
    H = g.message_generator()
    raw = api.elgamal_message_generator(sg)
    assert api.serialize(g.group, [raw]) == [g.to_bytes(H)]
    assert api.elgamal_message_generator(sg, api.FMT_COMPRESSED) == g.to_bytes(H)
    assert api.elgamal_message_generator(sg, api.FMT_RAW_AFFINE) == g.aff_raw(H)
    assert api.elgamal_message_generator(sg) == raw          # cached: the same bytes again


@pytest.mark.parametrize('sg', [1, 2])
def test_case_list_flat_call(api, sg):
    """Every case, explicit generators (the default one passed as a point), a key per proof, points under random Z."""
    rng = random.Random(sg)
    cl = ec.cases(sg)
    pks, gens, c1s, c2s, mps, bps, chs = ec.arrays(sg, cl, rng)
    got = api.elgamal_proof_verify_batch(sg, pks, gens, c1s, c2s, mps, bps, chs)
    assert got == [cs.expect for cs in cl], names(cl, got)
    # generators = NULL: the cases that use the message generator
    dl = [cs for cs in cl if cs.generator is ec.DEFAULT]
    pks, gens, c1s, c2s, mps, bps, chs = ec.arrays(sg, dl, rng, explicit_generators=False)
    got = api.elgamal_proof_verify_batch(sg, pks, None, c1s, c2s, mps, bps, chs)
    assert got == [cs.expect for cs in dl], names(dl, got)
    assert {api.elgamal_error_from_status(s).msg for s in (16, 17, 18)} == set(ec.ERRORS.values())
    assert [api.elgamal_error_from_status(s).msg for s in (16, 17, 18)] == [ec.ERRORS[s] for s in (16, 17, 18)]
    assert api.elgamal_error_from_status(0) is None and api.elgamal_error_from_status(7) == api.BlsError('DeserializationError')


@pytest.mark.parametrize('sg', [1, 2])
def test_case_list_tensor_ops(api, sg):
    import torch
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    rng = random.Random(10 + sg)
    cl = ec.cases(sg)
    pks, gens, c1s, c2s, mps, bps, chs = ec.arrays(sg, cl, rng)
    tens = lambda b: torch.tensor(list(b), dtype=torch.uint8, device=dev)
    sc = lambda xs: tens(b''.join(int(x).to_bytes(32, 'little') for x in xs))
    st = ops.elgamal_proof_verify_batch(sg, tens(b''.join(pks)), len(cl), tens(b''.join(gens)), tens(b''.join(c1s)), tens(b''.join(c2s)), sc(mps), sc(bps),
                                        sc(chs), len(cl))
    assert st.is_cuda and st.tolist() == [cs.expect for cs in cl], names(cl, st.tolist())
    g = ec.kg(sg)
    assert api.serialize(g.group, [bytes(ops.elgamal_message_generator(sg).tolist())]) == [g.to_bytes(g.message_generator())]


def cycle(cl, n):
    return [cl[i % len(cl)] for i in range(n)]


@pytest.mark.parametrize('n', [1, 2, 64, 65])
@pytest.mark.parametrize('sg', [1, 2])
def test_shapes(api, sg, n):
    """n = 1, 2, a full wave and one lane past it; a key per proof and one shared key; generators NULL and explicit."""
    rng = random.Random(100 * sg + n)
    cl = ec.cases(sg)
    honest_pk = cl[0].pk
    same_pk = [cs for cs in cl if cs.pk == honest_pk]
    for shared in (False, True):
        for explicit in (False, True):
            pool = [cs for cs in (same_pk if shared else cl) if explicit or cs.generator is ec.DEFAULT]
            assert len({cs.expect for cs in pool}) == 5          # every status stays in every sub-list
            sub = cycle(pool[::-1] if n > 2 else pool, n)
            pks, gens, c1s, c2s, mps, bps, chs = ec.arrays(sg, sub, rng, explicit_generators=explicit, shared_pk=honest_pk if shared else None)
            got = api.elgamal_proof_verify_batch(sg, pks, gens, c1s, c2s, mps, bps, chs)
            assert got == [cs.expect for cs in sub], (shared, explicit, names(sub, got))


@pytest.mark.parametrize('sg', [1, 2])
def test_input_formats_agree(api, sg):
    g = ec.kg(sg)
    cl = ec.cases(sg)
    H = g.message_generator()
    pts = lambda f: [[f(cs.pk) for cs in cl], [f(H if cs.generator is ec.DEFAULT else cs.generator) for cs in cl], [f(cs.c1) for cs in cl],
                     [f(cs.c2) for cs in cl]]
    scal = [[cs.mp for cs in cl], [cs.bp for cs in cl], [cs.ch for cs in cl]]
    want = [cs.expect for cs in cl]
    aff = lambda p: bytes(2 * g.K) if p is None else g.aff_raw(p)
    got = api.elgamal_proof_verify_batch(sg, *pts(aff), *scal, fmt=api.FMT_RAW_AFFINE)
    assert got == want, names(cl, got)
    got = api.elgamal_proof_verify_batch(sg, *pts(g.to_bytes), *scal, fmt=api.FMT_COMPRESSED)
    assert got == want, names(cl, got)
    # a point that does not decode is BAD_ENCODING whatever else is wrong with the proof; with one shared key it fails every proof
    comp = pts(g.to_bytes)
    bad = bytes([0xff]) * g.K
    comp[2][0] = bad
    comp[3][1] = bad
    got = api.elgamal_proof_verify_batch(sg, *comp, *scal, fmt=api.FMT_COMPRESSED)
    assert got[:2] == [7, 7] and got[2:] == want[2:]
    got = api.elgamal_proof_verify_batch(sg, [bad], *comp[1:], *scal, fmt=api.FMT_COMPRESSED)
    assert got == [7] * len(cl)


def test_argument_checks(api):
    lib = api.load_library()
    st = (ctypes.c_int32 * 4)(*[-77] * 4)
    p = ctypes.cast(st, ctypes.c_void_p)
    assert lib.blsgpu_elgamal_proof_verify_batch(1, None, 0, None, None, None, None, None, None, 0, 0, p) == 0
    assert list(st) == [-77] * 4
    buf = ctypes.create_string_buffer(3 * 288)
    b = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.blsgpu_elgamal_proof_verify_batch(1, b, 2, None, b, b, b, b, b, 3, 0, p) == -3
    assert lib.blsgpu_elgamal_proof_verify_batch(3, b, 3, None, b, b, b, b, b, 3, 0, p) == -3
    assert lib.blsgpu_elgamal_proof_verify_batch(1, b, 3, None, b, b, b, b, b, 3, 4, p) == -3
    assert list(st) == [-77] * 4
    assert lib.blsgpu_elgamal_open_batch(1, None, None, None, None, 0, 0, None, None) == 0
    assert lib.blsgpu_elgamal_open_batch(1, b, b, b, None, 1, 0, b, p) == -3          # ids without offsets
    assert lib.blsgpu_elgamal_open_batch(1, b, None, b, None, 1, 2, b, p) == -3       # wire format


@pytest.mark.parametrize('sg', [1, 2])
def test_open_batch_ragged(api, sg):
    """An empty set, a one-share set, a duplicate identifier, an identifier >= r, and good sets of 2, 3 and 5 shares in one call:
    the statuses of combine_shares, and c2 - key checked in the oracle."""
    g = ec.kg(sg)
    rng = random.Random(40 + sg)
    pt = lambda: g.mul(g.gen, rng.randrange(1, R))
    sets = []
    for t in (2, 0, 1, 3, 2, 5, 2, 2):
        sets.append([(rng.randrange(1, R), pt()) for _ in range(t)])
    sets[4][1] = (sets[4][0][0], sets[4][1][1])       # duplicate identifier
    sets[6][0] = (R, sets[6][0][1])                   # no Scalar
    sets[7] = [(1, pt()), (2, None)]                  # an identity share is a share like any other
    c2s = [pt() for _ in sets]
    c2s[3] = None
    want = [ec.from_shares(g, s) for s in sets]
    assert [w[0] for w in want] == [0, 13, 13, 0, 13, 0, 7, 0]
    raw_sets = [[(i, g.raw(p, rng)) for i, p in s] for s in sets]
    out, st = api.elgamal_open_batch(sg, [g.raw(p, rng) for p in c2s], raw_sets)
    assert st == [w[0] for w in want]
    exp = [g.to_bytes(ec.decrypt(g, w[1], c2) if w[0] == 0 else None) for w, c2 in zip(want, c2s)]
    assert api.serialize(g.group, out) == exp
    # the same keys from combine_shares, then the plain decrypt door
    keys, kst = api.combine_shares(g.group, [[(i, p, None) for i, p in s] for s in raw_sets])
    assert kst == st
    good = [k for k in range(len(sets)) if st[k] == 0]
    out2 = api.elgamal_decrypt_batch(sg, [g.raw(c2s[k], rng) for k in good], [keys[k] for k in good])
    assert api.serialize(g.group, out2) == [exp[k] for k in good]
    # c2 = key: the identity leaves as all-zero bytes
    out3 = api.elgamal_decrypt_batch(sg, [keys[0]], [keys[0]])
    assert out3 == [bytes(len(keys[0]))]
    # RAW_AFFINE input gives the same
    aff = lambda p: bytes(2 * g.K) if p is None else g.aff_raw(p)
    out4, st4 = api.elgamal_open_batch(sg, [aff(p) for p in c2s], [[(i, aff(p)) for i, p in s] for s in sets], fmt=api.FMT_RAW_AFFINE)
    assert st4 == st and api.serialize(g.group, out4) == exp


@pytest.mark.parametrize('sg', [1, 2])
def test_open_batch_tensor_ops(api, sg):
    import torch
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    g = ec.kg(sg)
    rng = random.Random(50 + sg)
    pt = lambda: g.mul(g.gen, rng.randrange(1, R))
    sets = [[(rng.randrange(1, R), pt()) for _ in range(t)] for t in (3, 1, 2)]
    c2s = [pt() for _ in sets]
    tens = lambda b: torch.tensor(list(b), dtype=torch.uint8, device=dev)
    offs = [0]
    for s in sets:
        offs.append(offs[-1] + len(s))
    out, st = ops.elgamal_open_batch(sg, tens(b''.join(g.raw(p, rng) for p in c2s)), len(sets),
                                     tens(b''.join(i.to_bytes(32, 'little') for s in sets for i, _ in s)),
                                     tens(b''.join(g.raw(p, rng) for s in sets for _, p in s)), torch.tensor(offs, dtype=torch.int64, device=dev))
    assert out.is_cuda and st.tolist() == [0, 13, 0]
    osz = 144 * g.group
    raw = bytes(out.tolist())
    want = [ec.from_shares(g, s) for s in sets]
    assert api.serialize(g.group, [raw[osz * k:osz * (k + 1)] for k in range(3)]) == \
        [g.to_bytes(ec.decrypt(g, w[1], c2) if w[0] == 0 else None) for w, c2 in zip(want, c2s)]


@pytest.mark.parametrize('sg', [1, 2])
def test_elgamal_ciphertext_works(api, pkg, sg):
    """The reference's elgamal_ciphertext_works through the wrapper types: three ciphertexts to one key, each with its proof; their sum
    opened from threshold shares of the key is the message generator times the sum of the messages."""
    g = ec.kg(sg)
    impl = pkg.api.Bls12381G1Impl if sg == 1 else pkg.api.Bls12381G2Impl
    rng = random.Random(60 + sg)
    sk, a1 = rng.randrange(1, R), rng.randrange(1, R)
    pk_pt = g.mul(g.gen, sk)
    pk = api.PublicKey(impl, g.raw(pk_pt, rng))
    ms = [rng.randrange(1, 1000) for _ in range(3)]
    proofs, pts = [], []
    for m in ms:
        c1, c2, mp, bp, ch = ec.seal_scalar_with_proof(g, pk_pt, m, ec.DEFAULT, rng.randrange(1, R), rng.randrange(1, R))
        pts.append((c1, c2))
        proofs.append(api.ElGamalProof(api.ElGamalCiphertext(impl, g.raw(c1, rng), g.raw(c2, rng)), mp, bp, ch))
    for pr in proofs:
        pr.verify(pk)
    assert api.elgamal_verify_many([(pr, pk) for pr in proofs]) == [None] * 3
    bad = api.ElGamalProof(proofs[0].ciphertext, proofs[0].message_proof, proofs[0].blinder_proof, (proofs[0].challenge + 1) % R)
    with pytest.raises(api.BlsError) as ei:
        bad.verify(pk)
    assert ei.value == api.BlsError('InvalidInputs', 'Challenge values do not match')
    total = proofs[0].ciphertext + proofs[1].ciphertext + proofs[2].ciphertext
    c1 = None
    for a, _ in pts:
        c1 = g.add(c1, a)
    assert api.serialize(g.group, [total.c1]) == [g.to_bytes(c1)]
    shares = [api.ElGamalDecryptionShare(impl, x, g.raw(g.mul(c1, (sk + a1 * x) % R), rng)) for x in (1, 2, 3)]
    key = api.ElGamalDecryptionKey.from_shares(shares[1:])
    assert api.serialize(g.group, [key.decrypt(total)]) == [g.to_bytes(g.mul(g.message_generator(), sum(ms)))]
    with pytest.raises(api.BlsError) as ei:
        api.ElGamalDecryptionKey.from_shares(shares[:1])
    assert ei.value == api.BlsError('VsssError')
    out, st = api.elgamal_open_batch(sg, [total.c2], [[(s.identifier, s.raw) for s in shares]])
    assert st == [0] and api.serialize(g.group, out) == [g.to_bytes(g.mul(g.message_generator(), sum(ms)))]
