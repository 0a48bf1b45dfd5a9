"""The two-pair "doors" of the C ABI that share run_pairing2 -- blsgpu_sig_proof_verify_batch, blsgpu_pop_verify_batch,
blsgpu_signcrypt_valid_batch, blsgpu_core_verify, blsgpu_core_verify_hashed, blsgpu_pairing2_check_batch -- as a list of items
and the result the reference gives each of them.  CPU only, every expectation from the oracle (oracle/py), none from the library.

Per orientation and door a POOL of base items (message / V lengths from MSG_LENS, `msg_len`: with a 48- or 96-byte key prefix
in front these fall on both sides of a SHA-256 block edge); every kind of KINDS[door] is derived from every base item and its
expected result computed once (items of a batch are independent, so a batch of thousands repeats them):

  sig_proof, pop, core_verify, hashed   a status of include/blsgpu.h, from ref.sig_proof_verify / ref.pop_verify / ref.core_verify
                                        (hashed: core_verify's order restated on a given message point, `hashed_core_verify`)
  signcrypt, pairing2                   a bool (the reference returns a Choice / is_identity()), from ref.signcrypt_valid /
                                        c.pairing_product_is_one

An item is a tuple of abstract columns (COLS[door]): oracle points, a challenge, bytes.  `build_batch` tiles the pool to n items,
puts failing items where the kernels change plan (`pinned_sites`) and renders every occurrence afresh -- a new Jacobian Z for
RAW_PROJ, or the affine form -- so a repeated pool item is never byte-identical.  tests/test_pairing_door_cases.py checks the
list on the CPU; tests/test_gpu_pairing_doors.py runs the batches on the device; tests/test_hostsim_pairing_doors.py runs the
items through the host copy of the prepare bodies with the bound tracker on."""
import functools
import hashlib
import random

import util
from oracle.py import bls381 as c
from oracle.py import blsful_ref as ref

RAW_PROJ, RAW_AFFINE = 0, 1                               # include/blsgpu.h
OK, INVALID_SIGNATURE, SIG_IDENTITY, PK_IDENTITY = 0, 1, 2, 3
COMMITMENT_IDENTITY, PROOF_IDENTITY, ZERO_CHALLENGE = 9, 10, 11
IMPLS = {1: ref.G1Impl, 2: ref.G2Impl}                    # sig_group -> orientation
SCHEMES = (ref.BASIC, ref.AUG, ref.POP)
MSG_LENS = (0, 1, 55, 56, 64, 119, 200)
POOL = 3                                                  # base items per (door, orientation, scheme): kept small, the oracle is slow
CORE_DST = b'PAIRING-DOORS-EXPLICIT-DST-V01_'             # blsgpu_core_verify: differs from every scheme's DST and the PoP DST

DOORS = ('sig_proof', 'pop', 'signcrypt', 'core_verify', 'hashed', 'pairing2')
# column types: S / K a point of the signature / key group of the orientation, 1 / 2 a point of G1 / G2, y a challenge (int),
# m bytes (message or V)
COLS = {'sig_proof': 'SSKym',      # commitment U, proof V, pk, y, msg
        'pop': 'KS',               # pk, proof
        'signcrypt': 'KSm',        # U, W, V
        'core_verify': 'KSm',      # pk, sig, msg
        'hashed': 'KSS',           # pk, sig, H(m)
        'pairing2': '1212'}        # g1a, g2a, g1b, g2b
HAS_SCHEME = {'sig_proof', 'signcrypt'}
HAS_FMT = {'sig_proof', 'pop', 'signcrypt', 'core_verify', 'pairing2'}      # core_verify_hashed takes RAW_PROJ only
BOOL_DOORS = {'signcrypt', 'pairing2'}
# what include/blsgpu.h lists per door (bool doors: both verdicts)
STATUS_CLASSES = {'sig_proof': {OK, INVALID_SIGNATURE, COMMITMENT_IDENTITY, PROOF_IDENTITY, PK_IDENTITY, ZERO_CHALLENGE},
                  'pop': {OK, INVALID_SIGNATURE, SIG_IDENTITY, PK_IDENTITY},
                  'core_verify': {OK, INVALID_SIGNATURE, SIG_IDENTITY, PK_IDENTITY},
                  'hashed': {OK, INVALID_SIGNATURE, SIG_IDENTITY, PK_IDENTITY},
                  'signcrypt': {True, False}, 'pairing2': {True, False}}

KINDS = {
    'sig_proof': ('valid', 'y_plus_1', 'msg_flip', 'other_key', 'other_dst', 'u_inf', 'v_inf', 'pk_inf', 'y_zero', 'all_four',
                  'y_one', 'y_r_minus_1', 't_inf', 'u_eq_yh'),
    'pop': ('valid', 'other_proof', 'sign_dst', 'pk_inf', 'proof_inf', 'both_inf'),
    'signcrypt': ('valid', 'v_flip', 'v_empty', 'other_w', 'other_dst', 'u_inf', 'w_inf', 'both_inf'),
    'core_verify': ('valid', 'msg_flip', 'other_key', 'other_sig', 'scheme_dst', 'pk_inf', 'sig_inf', 'both_inf'),
    'hashed': ('valid', 'other_hash', 'sig_inf', 'pk_inf', 'both_inf', 'h_inf'),
    'pairing2': ('one', 'not_one', 'off_g1a', 'off_g2a', 'off_g1b', 'off_g2b', 'both_trivial', 'inf_g1a', 'inf_g2a', 'inf_g1b',
                 'inf_g2b', 'three_inf', 'four_inf'),
}
# the kinds the prepare kernel itself gives a failure status (it leaves the item's pair slots unwritten): the stale-pairs test
PREPARE_FAILS = {'sig_proof': ('u_inf', 'v_inf', 'pk_inf', 'y_zero', 'all_four', 't_inf'), 'pop': ('pk_inf', 'proof_inf', 'both_inf'),
                 'signcrypt': ('u_inf', 'w_inf', 'both_inf'), 'core_verify': ('pk_inf', 'sig_inf', 'both_inf'),
                 'hashed': ('sig_inf', 'pk_inf', 'both_inf'), 'pairing2': ('inf_g1a', 'inf_g2a', 'inf_g1b', 'inf_g2b')}
# the kinds without an identity member: the cross-door comparisons
NO_IDENTITY = {'sig_proof': ('valid', 'y_plus_1', 'msg_flip', 'other_key', 'other_dst', 'y_one', 'y_r_minus_1', 'u_eq_yh'),
               'pop': ('valid', 'other_proof', 'sign_dst'), 'hashed': ('valid', 'other_hash')}


# ------------------------------------------------------------------ the oracle's side
def _status_of(fn, *args):
    try:
        fn(*args)
        return OK
    except ref.BlsError as e:
        if e.kind in ('InvalidSignature', 'InvalidProof'):
            return INVALID_SIGNATURE
        assert e.kind == 'InvalidInputs', e
        return {'signature is the identity point': SIG_IDENTITY, 'public key is the identity point': PK_IDENTITY,
                'commitment is the identity point': COMMITMENT_IDENTITY, 'proof is the identity point': PROOF_IDENTITY,
                'pk is the identity point': PK_IDENTITY, 'y is the zero': ZERO_CHALLENGE}[e.msg]


def hashed_core_verify(C, pk, sig, h):
    """ref.core_verify (sig_core.rs:120-146) with the message point given instead of hashed: the identity checks in its order, then
    the same pairing product -- where a pair with an identity member contributes 1 (c.miller_loop skips it, as the reference's
    multi_miller_loop does)."""
    if sig is None:
        raise ref.InvalidInputs('signature is the identity point')
    if pk is None:
        raise ref.InvalidInputs('public key is the identity point')
    if C.pairing_is_identity([(h, pk), (sig, C.pk_curve.neg(C.pk_gen))]):
        return
    raise ref.InvalidSignature


def expected(door, sg, scheme, item):
    """the reference's result for one abstract item of a door"""
    C = IMPLS.get(sg)
    if door == 'sig_proof':
        u, v, pk, y, msg = item
        return _status_of(ref.sig_proof_verify, C, u, v, pk, y, msg, C.DST[scheme])
    if door == 'pop':
        return _status_of(ref.pop_verify, C, *item)
    if door == 'signcrypt':
        u, w, v = item
        return bool(ref.signcrypt_valid(C, u, v, w, C.DST[scheme]))
    if door == 'core_verify':
        pk, sig, msg = item
        return _status_of(ref.core_verify, C, pk, sig, msg, CORE_DST)
    if door == 'hashed':
        return _status_of(hashed_core_verify, C, *item)
    assert door == 'pairing2', door
    g1a, g2a, g1b, g2b = item
    return bool(c.pairing_product_is_one([(g1a, g2a), (g1b, g2b)]))


def failed(want):
    """an expected result that is not 'accepted' (statuses: non-zero; bools: False)"""
    return want is False or (want is not True and want != OK)


# ------------------------------------------------------------------ the pools
def _scalar(*tag):
    return int.from_bytes(hashlib.sha512(repr(tag).encode()).digest(), 'big') % (c.R - 1) + 1          # 1 .. r - 1


def msg_len(t, j):
    """the length of base item j's message in the pool numbered t (sig_group + scheme; the hashed door: sig_group + 2): every
    second entry of MSG_LENS, starting at t, so the pools of a door -- core_verify and hashed taken together -- use every length"""
    return MSG_LENS[(t + 2 * j) % len(MSG_LENS)]


def _msg(tag, t, j):
    return (hashlib.sha512(b'door-msg-%s-%d-%d' % (tag.encode(), t, j)).digest() * 4)[:msg_len(t, j)]


def _flip(m):
    """a flipped bit of the last byte; the empty message has none and gets one byte instead"""
    return m[:-1] + bytes([m[-1] ^ 1]) if m else b'\x80'


@functools.lru_cache(maxsize=None)
def keys(sg):
    """POOL (secret key, public key) of an orientation, the same for every door"""
    C = IMPLS[sg]
    sks = [ref.keygen_from_hash(hashlib.sha256(b'door-key-%d-%d' % (sg, j)).digest()) for j in range(POOL)]
    return tuple((sk, ref.public_key(C, sk)) for sk in sks)


def _proof(C, sk, msg, dst, x, y):
    sig = C.sig_curve.mul(C.hash_to_point(msg, dst), sk)           # the message is hashed as given (no key prefix)
    return ref.sig_proof_generate(C, sig, msg, dst, x, y)


def _sig_proof_items(sg, scheme):
    C = IMPLS[sg]
    dst = C.DST[scheme]
    other = C.DST[SCHEMES[(SCHEMES.index(scheme) + 1) % 3]]
    out = {}
    for j, (sk, pk) in enumerate(keys(sg)):
        msg = _msg('proof', sg + scheme, j)
        x, y = _scalar('x', sg, scheme, j), _scalar('y', sg, scheme, j)
        assert y < c.R - 1 and (x + y) % c.R and (x + 1) % c.R and x != 1 and 2 * y % c.R     # y + 1 canonical, every V finite
        u, v = _proof(C, sk, msg, dst, x, y)
        out['valid', j] = (u, v, pk, y, msg)
        out['y_plus_1', j] = (u, v, pk, y + 1, msg)
        out['msg_flip', j] = (u, v, pk, y, _flip(msg))
        out['other_key', j] = (u, v, keys(sg)[(j + 1) % POOL][1], y, msg)
        out['other_dst', j] = _proof(C, sk, msg, other, x, y) + (pk, y, msg)
        out['u_inf', j] = (None, v, pk, y, msg)
        out['v_inf', j] = (u, None, pk, y, msg)
        out['pk_inf', j] = (u, v, None, y, msg)
        out['y_zero', j] = (u, v, pk, 0, msg)
        out['all_four', j] = (None, None, None, 0, msg)
        out['y_one', j] = _proof(C, sk, msg, dst, x, 1) + (pk, 1, msg)
        out['y_r_minus_1', j] = _proof(C, sk, msg, dst, x, c.R - 1) + (pk, c.R - 1, msg)
        # T = U + y H(m) is the identity: U = x H(m), y = -x (V any finite point)
        out['t_inf', j] = (u, v, pk, c.R - x, msg)
        # U = y H(m): a valid proof made with x = y, whose U + y H(m) is a doubling
        out['u_eq_yh', j] = _proof(C, sk, msg, dst, y, y) + (pk, y, msg)
    return out


def _pop_items(sg):
    C = IMPLS[sg]
    proofs = [ref.pop_prove(C, sk) for sk, _ in keys(sg)]
    out = {}
    for j, (sk, pk) in enumerate(keys(sg)):
        out['valid', j] = (pk, proofs[j])
        out['other_proof', j] = (pk, proofs[(j + 1) % POOL])
        out['sign_dst', j] = (pk, ref.sign(C, ref.POP, sk, C.pk_to_bytes(pk)))          # the signing DST, not the PoP one
        out['pk_inf', j] = (None, proofs[j])
        out['proof_inf', j] = (pk, None)
        out['both_inf', j] = (None, None)
    return out


def _signcrypt_items(sg, scheme):
    C = IMPLS[sg]
    dst = C.DST[scheme]
    other = C.DST[SCHEMES[(SCHEMES.index(scheme) + 1) % 3]]
    base = []
    for j in range(POOL):
        r = _scalar('signcrypt', sg, scheme, j)
        u = C.pk_curve.mul(C.pk_gen, r)                                        # U = P^r              sign_crypt.rs:46
        v = _msg('ct', sg + scheme, j)                                   # V: opaque to the validity check
        w = C.sig_curve.mul(ref.signcrypt_compute_w(C, u, v, dst), r)          # W = H(U || V)^r      sign_crypt.rs:59
        base.append((r, u, v, w))
    out = {}
    for j, (r, u, v, w) in enumerate(base):
        out['valid', j] = (u, w, v)
        out['v_flip', j] = (u, w, _flip(v))
        out['v_empty', j] = (u, w, b'')                       # the base item whose V is empty stays valid: the oracle decides
        out['other_w', j] = (u, base[(j + 1) % POOL][3], v)
        out['other_dst', j] = (u, C.sig_curve.mul(ref.signcrypt_compute_w(C, u, v, other), r), v)
        out['u_inf', j] = (None, w, v)
        out['w_inf', j] = (u, None, v)
        out['both_inf', j] = (None, None, v)
    return out


def _core_verify_items(sg):
    C = IMPLS[sg]
    out = {}
    sigs = []
    for j, (sk, pk) in enumerate(keys(sg)):
        msg = _msg('core', sg, j)
        sigs.append((msg, C.sig_curve.mul(C.hash_to_point(msg, CORE_DST), sk)))
    for j, (sk, pk) in enumerate(keys(sg)):
        msg, sig = sigs[j]
        out['valid', j] = (pk, sig, msg)
        out['msg_flip', j] = (pk, sig, _flip(msg))
        out['other_key', j] = (keys(sg)[(j + 1) % POOL][1], sig, msg)
        out['other_sig', j] = (pk, sigs[(j + 1) % POOL][1], msg)
        out['scheme_dst', j] = (pk, ref.sign(C, ref.BASIC, sk, msg), msg)      # signed under the Basic scheme's DST
        out['pk_inf', j] = (None, sig, msg)
        out['sig_inf', j] = (pk, None, msg)
        out['both_inf', j] = (None, None, msg)
    return out


@functools.lru_cache(maxsize=None)
def hashed_messages(sg):
    """the messages behind the 'hashed' door's points (hashed under the Basic scheme's DST), for the cross-door comparison"""
    return tuple(_msg('hashed', sg + 2, j) for j in range(POOL))


def _hashed_items(sg):
    C = IMPLS[sg]
    hs = [C.hash_to_point(m, C.DST[ref.BASIC]) for m in hashed_messages(sg)]
    out = {}
    for j, (sk, pk) in enumerate(keys(sg)):
        sig = C.sig_curve.mul(hs[j], sk)
        out['valid', j] = (pk, sig, hs[j])
        out['other_hash', j] = (pk, sig, hs[(j + 1) % POOL])
        out['sig_inf', j] = (pk, None, hs[j])
        out['pk_inf', j] = (None, sig, hs[j])
        out['both_inf', j] = (None, None, hs[j])
        out['h_inf', j] = (pk, sig, None)                      # a valid-looking key and signature beside H = identity
    return out


def _pairing2_items():
    g1, g2 = c.G1_GEN, c.G2_GEN
    out = {}
    for j in range(POOL):
        a, b, d = _scalar('p2a', j), _scalar('p2b', j), _scalar('p2d', j)
        e = a * b * pow(d, -1, c.R) % c.R                                      # e(a g1, b g2) e(-e g1, d g2) = 1  <=>  a b = e d
        sc = [a, b, c.R - e, d]
        assert all(0 < s < c.R - 1 for s in sc)                                # s + 1 is a canonical non-zero scalar too

        def pts(s):
            return (c.E1.mul(g1, s[0]), c.E2.mul(g2, s[1]), c.E1.mul(g1, s[2]), c.E2.mul(g2, s[3]))
        one = pts(sc)
        out['one', j] = one
        out['not_one', j] = pts([_scalar('p2n', j, k) for k in range(4)])
        for k, nm in enumerate(('g1a', 'g2a', 'g1b', 'g2b')):
            off = (c.E1 if k % 2 == 0 else c.E2).mul(g1 if k % 2 == 0 else g2, sc[k] + 1)
            out['off_' + nm, j] = one[:k] + (off,) + one[k + 1:]
            out['inf_' + nm, j] = one[:k] + (None,) + one[k + 1:]              # exactly one pair trivial
        # both pairs trivial: one identity in each pair, the members walking with j
        bt = list(one)
        bt[j % 2] = None
        bt[2 + (j // 2) % 2] = None
        out['both_trivial', j] = tuple(bt)
        th = [None] * 4
        th[j % 4] = one[j % 4]
        out['three_inf', j] = tuple(th)
        out['four_inf', j] = (None,) * 4
    return out


@functools.lru_cache(maxsize=None)
def cases(door, sg=0, scheme=0):
    """{(kind, j): (abstract item, expected result)} for every kind of the door and every base item j.  sg is 0 for 'pairing2',
    scheme 0 for the doors that take none."""
    assert (door == 'pairing2') == (sg == 0) and (scheme == 0 or door in HAS_SCHEME), (door, sg, scheme)
    items = {'sig_proof': lambda: _sig_proof_items(sg, scheme), 'pop': lambda: _pop_items(sg), 'signcrypt': lambda: _signcrypt_items(sg, scheme),
             'core_verify': lambda: _core_verify_items(sg), 'hashed': lambda: _hashed_items(sg), 'pairing2': _pairing2_items}[door]()
    assert set(items) == {(k, j) for k in KINDS[door] for j in range(POOL)}
    return {key: (it, expected(door, sg, scheme, it)) for key, it in items.items()}


def fail_keys(door, sg=0, scheme=0, kinds=None):
    """the (kind, j) whose expected result is a failure, base item by base item, kinds in turn (restricted to `kinds` when given)"""
    cs = cases(door, sg, scheme)
    return tuple((k, j) for j in range(POOL) for k in KINDS[door] if (kinds is None or k in kinds) and failed(cs[k, j][1]))


def valid_kind(door):
    return KINDS[door][0]


# ------------------------------------------------------------------ rendering
def _g1_affine(pt):
    return bytes(96) if pt is None else util.g1_aff_raw(pt)


def _g2_affine(pt):
    return bytes(192) if pt is None else util.g2_aff_raw(pt)


def render_point(group, pt, fmt, rng):
    """one occurrence of a point: RAW_PROJ with a fresh Jacobian Z (the identity: Z = 0), or RAW_AFFINE (the identity: all zero)"""
    if fmt == RAW_PROJ:
        return util.g1_raw(pt, rng) if group == 1 else util.g2_raw(pt, rng)
    assert fmt == RAW_AFFINE, fmt
    return _g1_affine(pt) if group == 1 else _g2_affine(pt)


def render(door, sg, item, fmt, rng):
    out = []
    for t, v in zip(COLS[door], item):
        if t in 'SK12':
            group = {'S': sg, 'K': 3 - sg, '1': 1, '2': 2}[t]
            out.append(render_point(group, v, fmt, rng))
        else:
            out.append(v)
    return tuple(out)


# ------------------------------------------------------------------ layouts
def boundaries(n):
    """every 32-item boundary inside a batch of n items: every 64-item one and the last 128-item one are among them"""
    return list(range(32, n, 32))


def pinned_sites(n):
    """where a failing item must sit: item 0, item n - 1 and both sides (b - 1, b) of every boundary"""
    return sorted({0, n - 1} | {p for b in boundaries(n) for p in (b - 1, b)})


def roles(n):
    """'F' (a failing kind) or 'V' (valid) or 'O' (any kind, in turn) per position: F at every pinned site, V at every other
    neighbour of a pinned site (so the two failing items of a boundary sit between valid ones, and items 0 and n - 1 have a
    valid neighbour), elsewhere V V O V F repeating"""
    sites = set(pinned_sites(n))
    r = ['VVOVF'[i % 5] for i in range(n)]
    for s in sites:
        for p in (s - 1, s + 1):
            if 0 <= p < n:
                r[p] = 'V'
    for s in sites:
        r[s] = 'F'
    return r


def check_roles(n, r):
    """every pinned site holds a failing item; the failing items around it are the two sides of a boundary at most (three where
    item n - 1 follows a boundary's two, as at n = 130) and have a valid item next to them (one or two items have no room for one)"""
    for s in pinned_sites(n):
        assert r[s] == 'F', (n, s)
        lo = hi = s
        while lo > 0 and r[lo - 1] == 'F':
            lo -= 1
        while hi < n - 1 and r[hi + 1] == 'F':
            hi += 1
        near = [r[p] for p in (lo - 1, hi + 1) if 0 <= p < n]
        assert (hi - lo < (3 if n % 32 == 2 else 2) and 'V' in near) or n <= 2, (n, s, lo, hi, near)


def build_batch(door, sg=0, scheme=0, n=1, seed=0, layout='cycle', fmt=RAW_PROJ, kinds=None):
    """(columns, expected results, (kind, j) names) of a batch of n items of a door; columns is one list per argument of COLS[door].
    layout 'cycle': n >= 4 as `roles` says, the F positions walking through the failing (kind, j), the O positions through every
    kind, base items taken in turn; n < 4 the kind list rotated by the seed (every kind alone, at item 0).
    'all_valid': n valid items.  'all_fail': every item one of PREPARE_FAILS (or of `kinds`), which the prepare kernel itself
    fails.  'all_but_one': the same with one valid item at a seeded position."""
    cs = cases(door, sg, scheme)
    ks = KINDS[door]
    if layout == 'cycle':
        fk = fail_keys(door, sg, scheme, kinds)
        if n < 4:
            names = [(ks[(seed + i) % len(ks)], (seed + i) % POOL) for i in range(n)]
        else:
            r = roles(n)
            check_roles(n, r)
            cnt = {'F': seed, 'O': seed}
            names = []
            for i in range(n):
                if r[i] == 'V':
                    names.append((ks[0], (3 * i + seed) % POOL))
                elif r[i] == 'F':
                    names.append(fk[cnt['F'] % len(fk)])
                    cnt['F'] += 1
                else:
                    names.append((ks[cnt['O'] % len(ks)], (3 * i + seed) % POOL))
                    cnt['O'] += 1
    else:
        fk = fail_keys(door, sg, scheme, kinds or PREPARE_FAILS[door])
        names = [fk[(seed + i) % len(fk)] for i in range(n)]
        if layout == 'all_but_one':
            names[random.Random(seed).randrange(n)] = (ks[0], seed % POOL)
        elif layout == 'all_valid':
            names = [(ks[0], (seed + i) % POOL) for i in range(n)]
        else:
            assert layout == 'all_fail', layout
    rng = random.Random((seed << 20) ^ n)
    rows = [render(door, sg, cs[nm][0], fmt, rng) for nm in names]
    cols = [[row[k] for row in rows] for k in range(len(COLS[door]))]
    return cols, [cs[nm][1] for nm in names], names


# ------------------------------------------------------------------ the sizes tests/test_gpu_pairing_doors.py runs
# wave and workgroup boundaries, BLSGPU_WIDE_MAX (512), run_verify_items' own branch for 513 .. 1,024 in sig_group 1,
# BLSGPU_COOP_MAX (4,096) and the lane-split kernels above it
SIZES = (1, 31, 33, 63, 65, 129, 512, 513, 1024, 1025, 4096, 4097)
PLAN_SIZES = (40, 130)
STALE_SIZES = (40, 600, 4200)                             # the engine, one wave per item, lane-split under the default knobs


def combos():
    """(door, sg, scheme) of every pool: the three schemes for the doors that take one"""
    out = []
    for door in DOORS:
        for sg in ((0,) if door == 'pairing2' else (1, 2)):
            for scheme in (SCHEMES if door in HAS_SCHEME else (0,)):
                out.append((door, sg, scheme))
    return out
