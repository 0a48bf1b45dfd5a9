"""What tests/timecrypt_ref.py and tests/timecrypt_cases.py claim, checked on the CPU with the oracle: the exported pairing value is the
cube of the textbook reduced pairing, bilinear and of order r; the byte form round-trips and Gt one is the stated constant; the case
list is what it says; and the reference's own time-lock tests (tests/encryption.rs:66-140) hold on the restated seal / unseal."""
import pytest

import timecrypt_cases as tc
import timecrypt_ref as tr
from util import c, ref


def test_final_exponentiation_is_the_cube_of_the_plain_power():
    """the chain the library runs against a plain f^((p^12 - 1) / r), on three pairs"""
    for a, b in tc.SCALARS[:2] + tc.SCALARS[6:7]:
        m = c.miller_loop([(tc.g1_mul(a), tc.g2_mul(b))])
        assert c.final_exponentiation(m) == c.f12_pow(c.final_exponentiation_naive(m), 3)


def test_bilinear_with_the_bytes_decoded_back():
    base = tr.gt_from_bytes(tc.expected(1, 1))
    assert base == tc.value(1, 1) and base != c.F12_ONE
    for a, b in tc.SCALARS:
        assert tr.gt_from_bytes(tc.expected(a, b)) == c.f12_pow(base, a * b % c.R), (a, b)


def test_order_r_and_negation():
    base = tc.value(1, 1)
    assert c.f12_pow(base, c.R) == c.F12_ONE
    a, b = tc.SCALARS[1]
    assert c.f12_mul(tc.value(a, b), tc.value(c.R - a, b)) == c.F12_ONE          # e(P, Q) e(-P, Q) = 1


def test_gt_one_is_the_stated_constant():
    assert tr.GT_ONE == bytes(47) + b'\x01' + bytes(528) and len(tr.GT_ONE) == tr.GT_BYTES
    assert tr.gt_bytes(tr.pairing_value(None, c.G2_GEN)) == tr.GT_ONE == tr.gt_bytes(tr.pairing_value(c.G1_GEN, None))
    assert tr.gt_from_bytes(tr.GT_ONE) == c.F12_ONE


def test_byte_order_is_real_then_imaginary_per_power_of_w():
    f = tuple((2 * k + 1, 2 * k + 2) for k in range(6))
    b = tr.gt_bytes(f)
    assert [int.from_bytes(b[48 * i:48 * i + 48], 'big') for i in range(12)] == list(range(1, 13))
    assert tr.gt_from_bytes(b) == f


def test_the_dozen_pairs_are_distinct_and_regular():
    assert len(tc.SCALARS) == 12 and len({tc.expected(a, b) for a, b in tc.SCALARS}) >= 11      # (r-1, 1) and (1, r-1) pair to one value
    for a, b in tc.SCALARS:
        assert c.E1.on_curve(tc.g1_mul(a)) and c.E2.on_curve(tc.g2_mul(b))


@pytest.mark.parametrize('fmt', tc.FMTS, ids=[tc.FMT_IDS[f] for f in tc.FMTS])
def test_special_items_are_what_they_say(fmt):
    names, g1s, g2s, want, st = tc.special_items(fmt)
    assert len(names) == len(g1s) == len(g2s) == len(want) == len(st)
    for nm, w, s in zip(names, want, st):
        assert (w == tc.ZERO_GT) == (s != tc.OK) == nm.startswith('undecodable'), nm
        assert (w == tr.GT_ONE) == nm.startswith('identity'), nm
    i, j = names.index('P'), names.index('-P')
    assert c.f12_mul(tr.gt_from_bytes(want[i]), tr.gt_from_bytes(want[j])) == c.F12_ONE
    if fmt in (tc.COMPRESSED, tc.LEGACY):
        assert {tc.BAD_ENCODING} <= set(st) <= {tc.OK, tc.BAD_ENCODING, tc.LEGACY_FORMAT}
        assert (tc.LEGACY_FORMAT in st) == (fmt == tc.LEGACY)
        for g, col in ((1, g1s), (2, g2s)):                 # every well-formed wire point decodes to the point it renders
            for nm, b in zip(names, col):
                if not nm.startswith('undecodable'):
                    assert tc.decode_status(g, b, fmt) == tc.OK, nm


# ------------------------------------------------------------------ the reference's tests restated (tests/encryption.rs:66-140)
IDENT = b'round 12345'


def _keys(seed):
    sk = ref.keygen_from_hash(bytes([seed]) * 32)
    return sk


@pytest.mark.parametrize('sg', [1, 2])
@pytest.mark.parametrize('scheme', [ref.BASIC, ref.AUG, ref.POP])
def test_round_trip_wrong_signature_and_scheme(sg, scheme):
    C = tr.IMPLS[sg]
    sk = _keys(3 + sg)
    pk = ref.public_key(C, sk)
    msg = b'time-lock message %d %d' % (sg, scheme)
    ct = tr.seal(C, pk, msg, IDENT, scheme, bytes([0x11 * (scheme + 1)]) * 32)
    sig = C.sig_curve.mul(C.hash_to_point(IDENT, C.DST[scheme]), sk)       # the signature over the identifier as such (no augmentation)
    assert tr.unseal(C, ct, sig, scheme) == (tr.OK, msg)
    other = C.sig_curve.mul(C.hash_to_point(b'round 12346', C.DST[scheme]), sk)
    # another round's signature opens a pseudo-random frame: None either way, by the length rule or by the check
    st, m = tr.unseal(C, ct, other, scheme)
    assert st in (tr.INVALID_SIGNATURE, tr.BAD_FRAME) and m is None
    assert tr.unseal(C, ct, sig, (scheme + 1) % 3) == (tr.INVALID_SCHEME, None)
    assert tr.unseal(C, ct, None, scheme) == (tr.SIG_IDENTITY, None)


def test_frame_rules():
    """an empty w and an unterminated varint give the EMPTY message and leave the verdict to the check; a length beyond the frame is
    BAD_FRAME; one that fills the frame is OK"""
    C = tr.IMPLS[1]
    sk = _keys(9)
    pk = ref.public_key(C, sk)
    scheme = ref.BASIC
    sig = C.sig_curve.mul(C.hash_to_point(IDENT, C.DST[scheme]), sk)
    alpha = bytes(range(32))
    assert tr.unseal(C, tr.seal_raw_frame(C, pk, IDENT, scheme, alpha, b''), sig, scheme) == (tr.OK, b'')
    assert tr.unseal(C, tr.seal_raw_frame(C, pk, IDENT, scheme, alpha, b'\x80' * 32), sig, scheme) == (tr.OK, b'')
    body = bytes(range(40, 71))
    assert tr.unseal(C, tr.seal_raw_frame(C, pk, IDENT, scheme, alpha, bytes([31]) + body, message=body), sig, scheme) == (tr.OK, body)
    assert tr.unseal(C, tr.seal_raw_frame(C, pk, IDENT, scheme, alpha, bytes([32]) + body, message=body), sig, scheme) == (tr.BAD_FRAME, None)
    for n in (0, 1, 30, 31, 32, 127, 128):
        m = bytes((7 * i + n) & 0xff for i in range(n))
        ct = tr.seal(C, pk, m, IDENT, scheme, alpha)
        assert len(ct[2]) == max(32, n + (1 if n < 128 else 2)) and tr.unseal(C, ct, sig, scheme) == (tr.OK, m)


@pytest.mark.parametrize('sg', [1, 2])
def test_every_case_has_the_status_the_list_states(sg):
    """the groups of one call: sizes 0, 1, 2 and 5 with empty groups, every message length, every status of the contract, the
    precedence pairs; and what rendering adds on the wire formats"""
    groups = tc.timelock_groups(sg)
    assert [len(g['items']) for g in groups[:5]] == [0, 1, 2, 5, 0] and not groups[-1]['items']
    assert {g['scheme'] for g in groups if g['items']} == {ref.BASIC, ref.AUG, ref.POP}
    items = {it['name']: (g, it) for g in groups for it in g['items']}
    for n in tc.MESSAGE_LENGTHS:
        st, m = items['message of %d bytes' % n][1]['want']
        assert st == tc.OK and len(m) == n
    assert {len(items['message of %d bytes' % n][1]['w']) for n in (165, 166, 167, 334, 335)} == {167, 168, 169, 336, 337}
    st = lambda nm: items[nm][1]['want'][0]  # noqa: E731
    assert st('one bit flipped in u') == st('one bit flipped in v') == st('one bit flipped in w') == st('one bit flipped in the signature') == tc.INVALID_SIGNATURE
    assert st('a signature of another round') in (tc.INVALID_SIGNATURE, tc.BAD_FRAME) and st('... and its w empty') == tc.INVALID_SIGNATURE
    assert st('identity signature') == tc.SIG_IDENTITY and st('identity u') == tc.PK_IDENTITY and st('scheme mismatch') == tc.INVALID_SCHEME
    assert {it['want'][0] for _, it in items.values()} == {tc.OK, tc.INVALID_SIGNATURE, tc.SIG_IDENTITY, tc.PK_IDENTITY, tc.INVALID_SCHEME, tc.BAD_FRAME}
    for _, it in items.values():
        assert (it['want'][1] is not None) == (it['want'][0] == tc.OK), it['name']
    for fmt in tc.FMTS:
        api_groups, msgs, sts = tc.render_groups(sg, groups, fmt)
        assert sum(len(g[2]) for g in api_groups) == len(msgs) == len(sts)
        wire = fmt in (tc.COMPRESSED, tc.LEGACY)
        assert (tc.BAD_ENCODING in sts) == wire and (tc.LEGACY_FORMAT in sts) == (fmt == tc.LEGACY)
    g, it = items['undecodable signature and u']
    assert tc.expected_item(sg, g, it, tc.LEGACY) == (tc.BAD_ENCODING, None)                 # u's status, not the signature's
    g, it = items['undecodable signature']
    assert tc.expected_item(sg, g, it, tc.LEGACY) == (tc.LEGACY_FORMAT, None)
    tiled = tc.tiled_groups(sg, 4097)
    assert sum(len(g['items']) for g in tiled) == 4097 and len(tiled) > 400
