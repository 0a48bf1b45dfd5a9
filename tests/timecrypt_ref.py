"""Time-lock decryption restated on the CPU: the pairing VALUE as Gt bytes (blsgpu_pairing_batch) and TimeCryptCiphertext's seal /
unseal (reference src/traits/time_crypt.rs:22-141, src/time_crypt_ciphertext.rs:38-50) with the oracle, hashlib and hmac.  Every
expectation of tests/test_timecrypt_cases.py, tests/test_hostsim_timecrypt.py and the GPU tests comes from here, none from the library.

Two facts fix the bytes (include/blsgpu.h):
  the value   Gt is final_exponentiation(miller_loop(..)) of the backend, whose hard part raises to 3 (p^4 - p^2 + 1) / r: the CUBE of
              the textbook reduced pairing.  oracle/py/bls381.py final_exponentiation is that chain; tests/test_timecrypt_cases.py
              holds it against final_exponentiation_naive ** 3, bilinearity and the order r.
  the bytes   ASSUMED: gt_bytes below is the ONE Python function that knows the order (its device twin: csrc/timecrypt.cuh
              coop_gt_bytes).

A point is an oracle affine point or None (the identity); a ciphertext is (u, v, w, scheme)."""
import hashlib

from oracle.py import bls381 as c
from oracle.py import blsful_ref as ref
from pok_timestamp_cases import hash_to_scalar
from signcrypt_cases import VARINT_MAX, varint, xor

OK, INVALID_SIGNATURE, SIG_IDENTITY, PK_IDENTITY = 0, 1, 2, 3
BAD_ENCODING, INVALID_SCHEME, BAD_FRAME = 7, 12, 15
GT_BYTES = 576
SALT = b'TIMELOCK_BLS12381_XOF:HKDF-SHA2-256_'               # src/traits/time_crypt.rs:13
IMPLS = {1: ref.G1Impl, 2: ref.G2Impl}


# ------------------------------------------------------------------ the pairing value
def gt_bytes(f):
    """Gt::to_bytes() as assumed: the six Fp2 coefficients over w^0 .. w^5 (the oracle's flat Fp12), each its real part, then its
    imaginary part, each part 48 bytes big-endian of the canonical residue."""
    return b''.join((x % c.P).to_bytes(48, 'big') for co in f for x in co)


def gt_from_bytes(b):
    assert len(b) == GT_BYTES
    v = [int.from_bytes(b[48 * i:48 * i + 48], 'big') for i in range(12)]
    assert all(x < c.P for x in v)
    return tuple((v[2 * k], v[2 * k + 1]) for k in range(6))


GT_ONE = gt_bytes(c.F12_ONE)


def pairing_value(P, Q):
    """Pairing::pairing(&[(P, Q)]) as an oracle Fp12: P in G1, Q in G2; an identity member gives one (multi_miller_loop skips it)"""
    if P is None or Q is None:
        return c.F12_ONE
    return c.final_exponentiation(c.miller_loop([(P, Q)]))


def pairing_of(C, sig_member, key_member):
    """e(sig-group point, key-group point) of the impl: Bls12381G2Impl swaps so that the G1 member comes first (src/helpers.rs:56)"""
    return pairing_value(sig_member, key_member) if C is ref.G1Impl else pairing_value(key_member, sig_member)


# ------------------------------------------------------------------ seal / unseal
def compute_v(k, x32):
    return xor(hashlib.sha256(gt_bytes(k)).digest(), x32)


def compute_w(alpha, data):
    return xor(hashlib.shake_128(alpha).digest(len(data)), data) if data else b''


def scalar_r(alpha, message):
    return hash_to_scalar(alpha + hashlib.sha256(message).digest(), SALT)


def seal_raw_frame(C, pk, ident, scheme, alpha, frame, message=b'', r=None):
    """the ciphertext whose opened frame is `frame` (any bytes), sealed with r = H(alpha || SHA-256(message)) unless r is given"""
    assert len(alpha) == 32
    r = scalar_r(alpha, message) if r is None else r
    k = pairing_of(C, C.hash_to_point(ident, C.DST[scheme]), C.pk_curve.mul(pk, r))
    return (C.pk_curve.mul(C.pk_gen, r), compute_v(k, alpha), compute_w(alpha, frame), scheme)


def frame_of(msg):
    """varint(len) || message, padded with zeros to 32 bytes (time_crypt.rs:63-68)"""
    f = varint(len(msg)) + msg
    return f + bytes(max(0, 32 - len(f)))


def seal(C, pk, msg, ident, scheme, alpha):
    """BlsTimeCrypt::seal with a chosen one-time secret: alpha is what alpha.to_repr() would be, 32 bytes"""
    return seal_raw_frame(C, pk, ident, scheme, alpha, frame_of(msg), message=msg)


def peek(frame):
    """the length prefix of an opened frame: None when no varint terminates within the frame or 19 bytes (the message is then EMPTY
    and the check goes on, time_crypt.rs:89-102 -- not the signcryption rule), else (overhead, len)"""
    value = 0
    for i in range(VARINT_MAX):
        if i >= len(frame):
            return None
        value |= (frame[i] & 0x7f) << (7 * i)
        if not frame[i] & 0x80:
            return i + 1, value % 2 ** 64
    return None


def unseal(C, ct, sig, sig_scheme):
    """(status, message or None) of TimeCryptCiphertext::decrypt(sig): status == OK <=> is_some(); the first of the failures in the
    order include/blsgpu.h gives them (decode failures exist only on the wire formats and are not modelled here)"""
    u, v, w, scheme = ct
    if scheme != sig_scheme:
        return INVALID_SCHEME, None
    if sig is None:
        return SIG_IDENTITY, None
    if u is None:
        return PK_IDENTITY, None
    alpha = compute_v(pairing_of(C, sig, u), v)
    frame = compute_w(alpha, w)
    message = b''
    pk = peek(frame)
    if pk is not None:
        overhead, n = pk
        if n > len(frame) - overhead:
            return BAD_FRAME, None
        message = frame[overhead:overhead + n]
    r = scalar_r(alpha, message)
    if r == 0 or C.pk_curve.mul(C.pk_gen, r) != u:
        return INVALID_SIGNATURE, None
    return OK, message
