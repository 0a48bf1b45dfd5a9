"""Timestamp proofs of knowledge -- blsgpu_hash_to_scalar, blsgpu_sig_proof_challenge_batch, blsgpu_sig_proof_timestamp_verify_batch
-- restated on the CPU, and the list of cases the tests run.  Every expectation comes from here and the oracle (oracle/py), none
from the library.

  hash_to_scalar(msg, salt)     scalar_from_hkdf_bytes, reference src/helpers.rs:9-26, with hmac / hashlib and Python integers; equal
                                to ref.keygen_from_hash under the key-generation salt (tests/test_pok_timestamp_cases.py).  A zero
                                result is returned as zero (the reference's loop on it cannot end).
  compute_y(C, u, t)            BlsSignatureProof::compute_y, src/traits/sig_proof.rs:38-46
  timestamp_verify(...)         verify_timestamp_proof, :145-166, as a status of include/blsgpu.h: the timeout rule first (t in the
                                future with a timeout given: E_ARG, where the reference panics), then ref.sig_proof_verify

One call has ONE now_ms and ONE timeout_ms, so every case is an item (u, v, pk, t, msg) and carries two expectations: under
(NOW, None) and under (NOW, TIMEOUT).  'future_no_timeout' is the item of 'future_with_timeout' read under (NOW, None)."""
import functools
import hashlib
import hmac
import random

import util
from oracle.py import bls381 as c
from oracle.py import blsful_ref as ref

RAW_PROJ, RAW_AFFINE, COMPRESSED, LEGACY = 0, 1, 2, 3       # include/blsgpu.h
OK, INVALID_SIGNATURE, PK_IDENTITY = 0, 1, 3
COMMITMENT_IDENTITY, PROOF_IDENTITY, ZERO_CHALLENGE = 9, 10, 11
E_ARG = -3
IMPLS = {1: ref.G1Impl, 2: ref.G2Impl}
SCHEMES = (ref.BASIC, ref.AUG, ref.POP)
POK_SALT = b'BLS_POK__BLS12381_XOF:HKDF-SHA2-256_'          # src/traits/sig_proof.rs:5
KEYGEN_SALT = b'BLS-SIG-KEYGEN-SALT-'                       # src/helpers.rs:7
NOW, TIMEOUT = 1_700_000_000_000, 60_000                    # milliseconds
U64_MAX = 2 ** 64 - 1
MODES = {'none': None, 'timeout': TIMEOUT}

KINDS = ('valid', 't_plus_1', 'msg_flip', 'other_key', 'u_inf', 'v_inf', 'pk_inf', 'at_limit', 'past_limit', 'past_limit_u_inf',
         'future_with_timeout', 't_zero', 't_max')
# what every kind is, per mode; 'future_no_timeout' is future_with_timeout under 'none'
WANT = {
    'valid': (OK, OK), 't_plus_1': (INVALID_SIGNATURE, INVALID_SIGNATURE), 'msg_flip': (INVALID_SIGNATURE, INVALID_SIGNATURE),
    'other_key': (INVALID_SIGNATURE, INVALID_SIGNATURE), 'u_inf': (COMMITMENT_IDENTITY, COMMITMENT_IDENTITY),
    'v_inf': (PROOF_IDENTITY, PROOF_IDENTITY), 'pk_inf': (PK_IDENTITY, PK_IDENTITY), 'at_limit': (OK, OK),
    'past_limit': (OK, INVALID_SIGNATURE), 'past_limit_u_inf': (COMMITMENT_IDENTITY, INVALID_SIGNATURE),
    'future_with_timeout': (OK, E_ARG), 't_zero': (OK, INVALID_SIGNATURE), 't_max': (OK, E_ARG),
}
# the kinds the timeout rule decides under (NOW, TIMEOUT)
TIMEOUT_RULED = ('past_limit', 'past_limit_u_inf', 'future_with_timeout', 't_zero', 't_max')


# ------------------------------------------------------------------ the restatement
def hash_to_scalar(msg, salt):
    prk = hmac.new(salt, msg + b'\x00', hashlib.sha256).digest()
    t1 = hmac.new(prk, b'\x00\x30\x01', hashlib.sha256).digest()
    t2 = hmac.new(prk, t1 + b'\x00\x30\x02', hashlib.sha256).digest()
    return int.from_bytes((t1 + t2)[:48], 'big') % c.R


def compute_y(C, u, t):
    return hash_to_scalar(C.sig_to_bytes(u) + t.to_bytes(8, 'little'), POK_SALT)


def timeout_status(t, now, timeout):
    """the rule alone: None where it leaves the item to the proof check"""
    if timeout is None:
        return None
    if t > now:
        return E_ARG
    return INVALID_SIGNATURE if now - t > timeout else None


def _status_of(fn, *args):
    try:
        fn(*args)
        return OK
    except ref.BlsError as e:
        if e.kind == 'InvalidProof':
            return INVALID_SIGNATURE
        assert e.kind == 'InvalidInputs', e
        return {'commitment is the identity point': COMMITMENT_IDENTITY, 'proof is the identity point': PROOF_IDENTITY,
                'pk is the identity point': PK_IDENTITY, 'y is the zero': ZERO_CHALLENGE}[e.msg]


def timestamp_verify(C, u, v, pk, t, now, timeout, msg, dst):
    late = timeout_status(t, now, timeout)
    if late is not None:
        return late
    return _status_of(ref.sig_proof_verify, C, u, v, pk, compute_y(C, u, t), msg, dst)


# ------------------------------------------------------------------ the cases
def _scalar(*tag):
    return int.from_bytes(hashlib.sha512(repr(tag).encode()).digest(), 'big') % (c.R - 1) + 1


@functools.lru_cache(maxsize=None)
def keys(sg):
    C = IMPLS[sg]
    sks = [ref.keygen_from_hash(hashlib.sha256(b'pok-key-%d-%d' % (sg, j)).digest()) for j in range(2)]
    return tuple((sk, ref.public_key(C, sk)) for sk in sks)


def make_proof(C, sk, msg, dst, x, t):
    """generate_timestamp_proof (sig_proof.rs:75-99) with x and t given: (U, V) = (x H(m), -(x + y) sig), y = compute_y(U, t)"""
    h = C.hash_to_point(msg, dst)
    u = C.sig_curve.mul(h, x)
    y = compute_y(C, u, t)
    assert y and (x + y) % c.R
    return u, C.sig_curve.neg(C.sig_curve.mul(h, sk * (x + y) % c.R))


@functools.lru_cache(maxsize=None)
def items(sg, scheme):
    """{kind: (u, v, pk, t, msg)}"""
    C = IMPLS[sg]
    dst = C.DST[scheme]
    (sk, pk), (_, pk2) = keys(sg)
    msg = (hashlib.sha512(b'pok-msg-%d-%d' % (sg, scheme)).digest() * 2)[:(0, 1, 55, 56, 64, 119)[3 * (sg - 1) + scheme]]
    x = _scalar('pok-x', sg, scheme)

    def proof(t):
        return make_proof(C, sk, msg, dst, x, t)
    t0 = NOW - 1000
    u, v = proof(t0)
    out = {'valid': (u, v, pk, t0, msg), 't_plus_1': (u, v, pk, t0 + 1, msg),
           'msg_flip': (u, v, pk, t0, msg[:-1] + bytes([msg[-1] ^ 1]) if msg else b'\x80'), 'other_key': (u, v, pk2, t0, msg),
           'u_inf': (None, v, pk, t0, msg), 'v_inf': (u, None, pk, t0, msg), 'pk_inf': (u, v, None, t0, msg)}
    for kind, t in (('at_limit', NOW - TIMEOUT), ('past_limit', NOW - TIMEOUT - 1), ('future_with_timeout', NOW + 1), ('t_zero', 0),
                    ('t_max', U64_MAX)):
        out[kind] = proof(t) + (pk, t, msg)
    out['past_limit_u_inf'] = (None,) + out['past_limit'][1:]
    assert tuple(out) and set(out) == set(KINDS)
    return out


@functools.lru_cache(maxsize=None)
def expected(sg, scheme, kind, mode):
    C = IMPLS[sg]
    u, v, pk, t, msg = items(sg, scheme)[kind]
    return timestamp_verify(C, u, v, pk, t, NOW, MODES[mode], msg, C.DST[scheme])


# ------------------------------------------------------------------ rendering
def render_point(group, pt, fmt, rng):
    """one occurrence of a point: RAW_PROJ with a fresh Jacobian Z, RAW_AFFINE, or its wire bytes"""
    if fmt == RAW_PROJ:
        return util.g1_raw(pt, rng) if group == 1 else util.g2_raw(pt, rng)
    if fmt == RAW_AFFINE:
        if pt is None:
            return bytes(96 * group)
        return util.g1_aff_raw(pt) if group == 1 else util.g2_aff_raw(pt)
    b = (c.g1_compress if group == 1 else c.g2_compress)(pt)
    return ref.modern_to_legacy(b) if fmt == LEGACY else b


def build_batch(sg, scheme, n, mode, fmt=RAW_PROJ, seed=0, kinds=KINDS):
    """n items, the kinds interleaved (item i is kinds[(i + seed) % len]), every occurrence rendered afresh:
    (us, vs, pks, ts, msgs), the expected statuses, the kinds"""
    its = items(sg, scheme)
    rng = random.Random((seed << 20) ^ n ^ (sg << 8) ^ scheme)
    names = [kinds[(i + seed) % len(kinds)] for i in range(n)]
    cols = ([], [], [], [], [])
    for nm in names:
        u, v, pk, t, msg = its[nm]
        cols[0].append(render_point(sg, u, fmt, rng))
        cols[1].append(render_point(sg, v, fmt, rng))
        cols[2].append(render_point(3 - sg, pk, fmt, rng))
        cols[3].append(t)
        cols[4].append(msg)
    return cols, [expected(sg, scheme, nm, mode) for nm in names], names


# ------------------------------------------------------------------ inputs of the hash tests
MSG_LENS = tuple(range(201))
SALTS = {'pok': POK_SALT, 'keygen': KEYGEN_SALT, 'long65': bytes(range(1, 66))}
SIZES = (1, 63, 64, 65, 130)                                # BLS_BLOCK is 64


def hash_inputs(n, seed):
    rng = random.Random(seed)
    return [rng.randbytes(rng.choice(MSG_LENS)) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def points(sg, count=6):
    """a few commitments of an orientation, the identity among them"""
    C = IMPLS[sg]
    gen = c.G1_GEN if sg == 1 else c.G2_GEN
    return tuple(C.sig_curve.mul(gen, _scalar('pok-pt', sg, j)) for j in range(count - 1)) + (None,)
