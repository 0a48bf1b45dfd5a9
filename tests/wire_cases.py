"""Wire-format inputs of blsgpu_verify_batch (BLSGPU_FMT_COMPRESSED / BLSGPU_FMT_LEGACY) and the status the reference gives each of
them -- CPU only, every expectation from the oracle (oracle/py), none from the library.

What a caller of the reference does with wire bytes is PublicKey::from_bytes[_with_mode], Signature::from_bytes[_with_mode], then
Signature::verify.  `expected_status` restates exactly that order: the key's decode error (DeserializationError -> 7,
LegacyFormatError -> 8) is the item's status whatever the signature holds, then the signature's, then ref.verify of the decoded
points (0 / 1 / 2 / 3, the mapping of tests/test_gpu_verify.py::test_batch_mixed_against_oracle).

A POOL of signed triples per (orientation, scheme) is made by the oracle; every item kind of `KIND_TABLE` is derived from every pool
triple, its expected status computed once and cached (items of a batch are independent, so a batch of thousands repeats them).
`build_batch` lays the kinds out so that decode failures sit next to valid items at the places where the kernels change plan.
tests/test_wire_cases.py asserts the coverage conditions; tests/test_gpu_wire.py runs the batches on the device."""
import functools
import hashlib
import random

from oracle.py import bls381 as c
from oracle.py import blsful_ref as ref

FMT_COMPRESSED, FMT_LEGACY = 2, 3                       # include/blsgpu.h
OK, INVALID_SIGNATURE, SIG_IDENTITY, PK_IDENTITY, BAD_ENCODING, LEGACY_FORMAT = 0, 1, 2, 3, 7, 8
IMPLS = {1: ref.G1Impl, 2: ref.G2Impl}                  # sig_group -> orientation
MSG_LENS = (0, 1, 31, 32, 33, 55, 56, 64, 100)          # around the SHA-256 block and padding boundaries
POOL = len(MSG_LENS)                                    # triples per (orientation, scheme): one per message length
SCAN = 64                                               # candidates an off-curve / off-subgroup scan may look at


# ------------------------------------------------------------------ the oracle's side
@functools.lru_cache(maxsize=None)
def _decompress(nbytes, b):
    """the oracle's checked decompression of a modern encoding, once per distinct encoding: (status, point)"""
    try:
        return OK, (c.g1_decompress if nbytes == 48 else c.g2_decompress)(b)
    except c.DecodeError:
        return BAD_ENCODING, None


def decode(nbytes, b, fmt):
    """(status, point) of from_bytes (FMT_COMPRESSED) / from_bytes_with_mode(Legacy) (FMT_LEGACY) on a 48-byte G1 or a 96-byte G2
    encoding: the header rules of the reference (ref.validate_modern / ref.legacy_to_modern, reference src/impls/legacy.rs) in
    front of the oracle's checked decompression, the same for keys and signatures of both orientations.  For the 48-byte keys and
    96-byte signatures of Bls12381G2Impl the oracle also restates the reference's functions themselves; `decode_via_ref` runs
    those, and tests/test_wire_cases.py holds the two against each other."""
    try:
        if fmt == FMT_LEGACY:
            b = ref.legacy_to_modern(b)
        else:
            ref.validate_modern(b[0], 'G1' if nbytes == 48 else 'G2')
    except ref.BlsError as e:
        return {'DeserializationError': BAD_ENCODING, 'LegacyFormatError': LEGACY_FORMAT}[e.kind], None
    return _decompress(nbytes, b)


def decode_via_ref(nbytes, b, fmt):
    """status of ref.pk_from_bytes_with_mode (48 bytes) / ref.sig_from_bytes_with_mode (96 bytes) of Bls12381G2Impl"""
    fn = ref.pk_from_bytes_with_mode if nbytes == 48 else ref.sig_from_bytes_with_mode
    try:
        fn(ref.G2Impl, b, ref.LEGACY if fmt == FMT_LEGACY else ref.MODERN)
        return OK
    except ref.BlsError as e:
        return {'DeserializationError': BAD_ENCODING, 'LegacyFormatError': LEGACY_FORMAT}[e.kind]


@functools.lru_cache(maxsize=None)
def verify_status(sg, scheme, pk, sig, msg):
    try:
        ref.verify(IMPLS[sg], scheme, pk, sig, msg)
        return OK
    except ref.BlsError as e:
        if e.kind == 'InvalidSignature':
            return INVALID_SIGNATURE
        assert e.kind == 'InvalidInputs'
        return SIG_IDENTITY if 'signature' in e.msg else PK_IDENTITY


def expected_status(sg, scheme, fmt, pkb, sigb, msg):
    """from_bytes of the key, from_bytes of the signature, verify: the first error is the item's status."""
    C = IMPLS[sg]
    st, pk = decode(C.PK_BYTES, pkb, fmt)
    if st:
        return st
    st, sig = decode(C.SIG_BYTES, sigb, fmt)
    if st:
        return st
    return verify_status(sg, scheme, pk, sig, msg)


# ------------------------------------------------------------------ the pool
@functools.lru_cache(maxsize=None)
def pool(sg, scheme):
    """POOL signed triples (pk bytes, sig bytes, msg, pk point, sig point, secret key), modern encoding; the keys are the same for the three
    schemes of an orientation.  Both y-sign bits occur among the keys and among the signatures (asserted)."""
    C = IMPLS[sg]
    out = []
    for j, ln in enumerate(MSG_LENS):
        sk = ref.keygen_from_hash(hashlib.sha256(b'wire-pool-%d-%d' % (sg, j)).digest())
        pk = ref.public_key(C, sk)
        msg = hashlib.sha512(b'wire-msg-%d-%d-%d' % (sg, scheme, j)).digest() * 2
        msg = msg[:ln]
        sig = ref.sign(C, scheme, sk, msg)
        out.append((C.pk_to_bytes(pk), C.sig_to_bytes(sig), msg, pk, sig, sk))
    for k in (0, 1):
        assert {t[k][0] & 0x20 for t in out} == {0, 0x20}, 'the pool needs both y-sign bits (sg %d scheme %d, %s)' % (sg, scheme, 'pk sig'.split()[k])
    return tuple(out)


# ------------------------------------------------------------------ crafted encodings (all built in the modern form first)
def _x_bytes(nbytes, x):
    """x coordinate -> big-endian bytes with no header bits (G2: c1 then c0)"""
    return x.to_bytes(48, 'big') if nbytes == 48 else x[1].to_bytes(48, 'big') + x[0].to_bytes(48, 'big')


def _x_of(nbytes, b):
    v = bytes([b[0] & 0x1f]) + b[1:]
    return int.from_bytes(v, 'big') if nbytes == 48 else (int.from_bytes(v[48:], 'big'), int.from_bytes(v[:48], 'big'))


def _hdr(b, bits):
    return bytes([b[0] & 0x1f | bits]) + b[1:]


@functools.lru_cache(maxsize=None)
def scan(nbytes, start, want):
    """the first x = start + k (k < SCAN, added to the Fp / the c0 coordinate) that has no point on the curve (want 'offcurve') or
    whose points lie outside the prime-order subgroup ('offsub'), as a modern encoding with the y-sign bit clear.  Raises when the
    bound is reached: no kind is dropped silently."""
    E = c.E1 if nbytes == 48 else c.E2
    x0 = _x_of(nbytes, start)
    for k in range(1, SCAN + 1):
        x = (x0 + k) % c.P if nbytes == 48 else ((x0[0] + k) % c.P, x0[1])
        y = c.fp_sqrt(E.rhs(x)) if nbytes == 48 else c.f2_sqrt(E.rhs(x))
        if want == 'offcurve':
            if y is None:
                return _hdr(_x_bytes(nbytes, x), 0x80)
        elif y is not None and not (c.g1_in_subgroup((x, y)) if nbytes == 48 else c.g2_in_subgroup((x, y))):
            return _hdr(_x_bytes(nbytes, x), 0x80)
    raise RuntimeError('no %s x within %d candidates of %s' % (want, SCAN, start.hex()))


def _x_ge_p(nbytes, j):
    """0x9f ff...: the x (G2: the c1 half, or for odd j the c0 half under a small c1) is 2^381 - 1 >= p"""
    if nbytes == 48 or j % 2 == 0:
        return bytes([0x9f]) + b'\xff' * (nbytes - 1)
    return bytes([0x80]) + bytes(46) + b'\x01' + b'\xff' * 48


def _x_eq_p(nbytes, j):
    pb = c.P.to_bytes(48, 'big')
    if nbytes == 48:
        return _hdr(pb, 0x80)
    return _hdr(pb + bytes(48), 0x80) if j % 2 == 0 else bytes([0x80]) + bytes(47) + pb


def _infinity(nbytes):
    return bytes([0xc0]) + bytes(nbytes - 1)


def _to_fmt(b, fmt):
    return ref.modern_to_legacy(b) if fmt == FMT_LEGACY else b


def _flip_sign(b, fmt):
    return bytes([b[0] ^ (0x80 if fmt == FMT_LEGACY else 0x20)]) + b[1:]


def _bad_header(b, fmt, v):
    """modern: the three header bits of a valid encoding replaced by 000, 010, 111; legacy: 0x20, 0x40, 0x60 set on a valid one"""
    if fmt == FMT_LEGACY:
        return bytes([ref.modern_to_legacy(b)[0] | (0x20, 0x40, 0x60)[v]]) + b[1:]
    return _hdr(b, (0x00, 0x40, 0xe0)[v])


def _variants(nbytes, b, fmt, j):
    """the crafted encodings of one point (modern bytes b) in wire format fmt"""
    v = {'valid': _to_fmt(b, fmt), 'ysign': _flip_sign(_to_fmt(b, fmt), fmt), 'inf': _infinity(nbytes),
         'x_ge_p': _to_fmt(_x_ge_p(nbytes, j), fmt), 'x_eq_p': _to_fmt(_x_eq_p(nbytes, j), fmt),
         'offcurve': _to_fmt(scan(nbytes, b, 'offcurve'), fmt), 'offsub': _to_fmt(scan(nbytes, b, 'offsub'), fmt),
         # 0xc0 then a stray bit: the lowest of the last byte, or (odd j) the highest of the middle byte (G2: of the c0 half)
         'c0_junk': bytes([0xc0]) + (bytes(nbytes - 2) + b'\x01' if j % 2 == 0 else bytes(nbytes // 2 - 1) + b'\x80' + bytes(nbytes - nbytes // 2 - 1)),
         'inf_sign': bytes([0xe0]) + bytes(nbytes - 1)}
    for k in range(3):
        v['hdr%d' % k] = _bad_header(b, fmt, k)
    return v


# kind -> (key variant, signature variant, message edit, status the issue's table fixes or None for "as the oracle says")
_POINT_FAILS = ('hdr0', 'hdr1', 'hdr2', 'x_ge_p', 'x_eq_p', 'offcurve', 'offsub', 'c0_junk', 'inf_sign')
KIND_TABLE = {
    'valid': ('valid', 'valid', None, OK),
    'msg_append': ('valid', 'valid', 'append', INVALID_SIGNATURE),
    'msg_flip': ('valid', 'valid', 'flip', INVALID_SIGNATURE),
    'sig_ysign': ('valid', 'ysign', None, INVALID_SIGNATURE),
    'pk_ysign': ('ysign', 'valid', None, INVALID_SIGNATURE),
    'sig_other': ('valid', 'other', None, INVALID_SIGNATURE),
    'pk_inf': ('inf', 'valid', None, PK_IDENTITY),
    'sig_inf': ('valid', 'inf', None, SIG_IDENTITY),
    'both_inf': ('inf', 'inf', None, SIG_IDENTITY),
}
for _v in _POINT_FAILS:
    KIND_TABLE['pk_' + _v] = (_v, 'valid', None, None)
    KIND_TABLE['sig_' + _v] = ('valid', _v, None, None)
KIND_TABLE['pk_bad_sig_inf'] = ('offcurve', 'inf', None, BAD_ENCODING)           # a key failure beside an infinity signature
KIND_TABLE['pk_inf_sig_bad'] = ('inf', 'x_ge_p', None, BAD_ENCODING)             # decode comes before the identity checks
KIND_TABLE['pk_hdr_sig_inf'] = ('hdr1', 'inf', None, None)
KIND_TABLE['pk_inf_sig_hdr'] = ('inf', 'hdr1', None, None)
LEGACY_ONLY = {'pk8_sig7': ('hdr0', 'x_ge_p', None, LEGACY_FORMAT),             # two different failures: the key's wins
               'pk7_sig8': ('offcurve', 'hdr2', None, BAD_ENCODING)}
DECODE_FAIL = (BAD_ENCODING, LEGACY_FORMAT)


def kinds(fmt):
    """the kind names of a format, in a fixed order that mixes decodable and undecodable items (a prefix is a mixture): one
    of the nine kinds whose encodings are all well-formed, then up to three of the others"""
    ok = list(KIND_TABLE)[:9]
    bad = list(KIND_TABLE)[9:] + (list(LEGACY_ONLY) if fmt == FMT_LEGACY else [])
    out = []
    while ok or bad:
        out += ok[:1] + bad[:3]
        ok, bad = ok[1:], bad[3:]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cases(sg, scheme, fmt):
    """{(kind, j): (pk bytes, sig bytes, msg, expected status)} for every kind of the format and every pool triple j"""
    C = IMPLS[sg]
    P = pool(sg, scheme)
    table = dict(KIND_TABLE, **(LEGACY_ONLY if fmt == FMT_LEGACY else {}))
    out = {}
    for j, (pkb, sigb, msg, _, _, _) in enumerate(P):
        pv = _variants(C.PK_BYTES, pkb, fmt, j)
        sv = _variants(C.SIG_BYTES, sigb, fmt, j)
        sv['other'] = _to_fmt(P[(j + 1) % POOL][1], fmt)
        for kind in kinds(fmt):
            kp, ks, edit, fixed = table[kind]
            m = msg
            if edit == 'append':
                m = msg + b'\x00'
            elif edit == 'flip':                                    # the empty message has no last bit: it gets one byte instead
                m = msg[:-1] + bytes([msg[-1] ^ 1]) if msg else b'\x80'
            want = expected_status(sg, scheme, fmt, pv[kp], sv[ks], m)
            assert fixed is None or want == fixed, (sg, scheme, fmt, kind, j, want, fixed)
            out[kind, j] = (pv[kp], sv[ks], m, want)
    return out


def fail_kinds(sg, scheme, fmt):
    """the kinds that fail to decode for every pool triple, in kind order"""
    cs = cases(sg, scheme, fmt)
    return tuple(k for k in kinds(fmt) if all(cs[k, j][3] in DECODE_FAIL for j in range(POOL)))


# ------------------------------------------------------------------ layouts
def pinned_sites(n):
    """the positions of a batch of n >= 64 items where a decode failure must sit next to a valid item: item 0, item n - 1, both
    sides of every 32-item (hence every 64-item) boundary below 256, both sides of the two ends of the last full 128-item block"""
    bounds = [b for b in range(32, 256, 32) if b < n]
    q = n // 128
    if q:
        bounds += [b for b in (128 * (q - 1), 128 * q) if 0 < b < n]
    return sorted({0, n - 1} | {p for b in bounds for p in (b - 1, b)})


def roles(n):
    """'F' (fails to decode), 'V' (valid) or 'O' (any other kind) per position.  Around every pinned site F and V alternate (F on
    even positions; the last two items are V, F), so every site belongs to an adjacent (F, V) pair; elsewhere V F V F O repeats:
    two fifths valid, two fifths undecodable."""
    r = ['VFVFO'[i % 5] for i in range(n)]
    for s in pinned_sites(n):
        for p in (s - 1, s, s + 1):
            if 0 <= p < n:
                r[p] = 'F' if p % 2 == 0 else 'V'
    r[n - 1] = 'F'
    r[n - 2] = 'V'
    return r


def check_roles(n, r):
    for s in pinned_sites(n):
        near = [r[p] for p in (s - 1, s + 1) if 0 <= p < n]
        assert r[s] in 'FV' and ('V' if r[s] == 'F' else 'F') in near, (n, s, r[max(0, s - 2):s + 3])
    assert r[0] == 'F' and r[1] == 'V' and r[n - 1] == 'F' and r[n - 2] == 'V', n


def build_batch(sg, scheme, fmt, n, seed=0, layout='cycle'):
    """(pks, sigs, msgs, expected statuses, kind names) of a batch of n wire items.
    layout 'cycle': n >= 64 as `roles` says, the F positions walking through the undecodable kinds, the O positions through all
    others, pool triples taken in turn; n < 64 a prefix of the kind list rotated by the seed.
    'all_fail': every item undecodable.  'all_but_one': the same with one valid item at a seeded position.  'all_valid': the
    valid items of the same pool triples (same messages, so the same sizes of everything) as the other two."""
    cs = cases(sg, scheme, fmt)
    ks = kinds(fmt)
    fk = fail_kinds(sg, scheme, fmt)
    other = tuple(k for k in ks if k not in fk and k != 'valid')
    if layout == 'cycle':
        if n < 64:
            names = [ks[(seed + i) % len(ks)] for i in range(n)]
        else:
            r = roles(n)
            check_roles(n, r)
            cnt = {'F': seed, 'O': seed}
            names = []
            for i in range(n):
                if r[i] == 'V':
                    names.append('valid')
                else:
                    lst = fk if r[i] == 'F' else other
                    names.append(lst[cnt[r[i]] % len(lst)])
                    cnt[r[i]] += 1
    else:
        names = [fk[(seed + i) % len(fk)] for i in range(n)]
        if layout == 'all_but_one':
            names[random.Random(seed).randrange(n)] = 'valid'
        elif layout == 'all_valid':
            names = ['valid'] * n
        else:
            assert layout == 'all_fail', layout
    items = [cs[k, (5 * i + seed) % POOL] for i, k in enumerate(names)]
    return ([t[0] for t in items], [t[1] for t in items], [t[2] for t in items], [t[3] for t in items], names)


# ------------------------------------------------------------------ the sizes tests/test_gpu_wire.py runs (checked on the CPU first)
# the thresholds blsgpu's run_verify_items / run_pairing2 branch on (BLSGPU_WIDE_MAX 512, 1,024, BLSGPU_COOP_MAX 4,096), wave and
# workgroup boundaries, and the sizes tests/test_gpu_api.py::test_verify_batch_ragged_sizes uses
SIZES = {1: (1, 2, 31, 32, 33, 64, 65, 127, 128, 129, 255, 257, 512, 513, 1024, 1025, 4096, 4097, 6145),
         2: (1, 2, 33, 65, 129, 513, 1025, 4097)}
SIZES_THIN = (1, 33, 513, 4097)                        # Basic and Aug
SIZES_OTHER = (40, 600, 700, 1000, 1001, 4200, 5000, 70001)   # stale pairs, plans, shards, device-resident, beyond one chunk


def place(batch, sg, scheme, fmt, pos, kind, j=0):
    """put the item (kind, pool triple j) at position pos of a batch (in place), with its expected status"""
    t = cases(sg, scheme, fmt)[kind, j]
    for col, v in zip(batch, t + (kind,)):
        col[pos] = v
