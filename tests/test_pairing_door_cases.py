"""CPU checks of tests/pairing_door_cases.py: every kind is what its name says, the reference functions give the result the
table below fixes for it, every status class of a door occurs, and the batch builder puts a failing item where it promises."""
import pytest

import pairing_door_cases as d
import util
from oracle.py import bls381 as c
from oracle.py import blsful_ref as ref

COMBOS = d.combos()
IDS = ['%s-g%d-s%d' % t for t in COMBOS]

# kind -> the result the issue's list fixes (None: whatever the oracle says, checked to be a failure or not below)
FIXED = {
    'sig_proof': {'valid': 0, 'y_plus_1': 1, 'msg_flip': 1, 'other_key': 1, 'other_dst': 1, 'u_inf': d.COMMITMENT_IDENTITY,
                  'v_inf': d.PROOF_IDENTITY, 'pk_inf': d.PK_IDENTITY, 'y_zero': d.ZERO_CHALLENGE, 'all_four': d.COMMITMENT_IDENTITY,
                  'y_one': 0, 'y_r_minus_1': 0, 't_inf': 1, 'u_eq_yh': 0},
    'pop': {'valid': 0, 'other_proof': 1, 'sign_dst': 1, 'pk_inf': d.PK_IDENTITY, 'proof_inf': d.SIG_IDENTITY, 'both_inf': d.SIG_IDENTITY},
    'signcrypt': {'valid': True, 'v_flip': False, 'v_empty': None, 'other_w': False, 'other_dst': False, 'u_inf': False, 'w_inf': False,
                  'both_inf': False},
    'core_verify': {'valid': 0, 'msg_flip': 1, 'other_key': 1, 'other_sig': 1, 'scheme_dst': 1, 'pk_inf': d.PK_IDENTITY,
                    'sig_inf': d.SIG_IDENTITY, 'both_inf': d.SIG_IDENTITY},
    'hashed': {'valid': 0, 'other_hash': 1, 'sig_inf': d.SIG_IDENTITY, 'pk_inf': d.PK_IDENTITY, 'both_inf': d.SIG_IDENTITY, 'h_inf': 1},
    'pairing2': {'one': True, 'not_one': False, 'off_g1a': False, 'off_g2a': False, 'off_g1b': False, 'off_g2b': False,
                 'both_trivial': True, 'inf_g1a': False, 'inf_g2a': False, 'inf_g1b': False, 'inf_g2b': False, 'three_inf': True,
                 'four_inf': True},
}


@pytest.mark.parametrize('door,sg,scheme', COMBOS, ids=IDS)
def test_results_and_classes(door, sg, scheme):
    """the oracle's result of every (kind, base item) is the one the list fixes; every class the header lists for the door occurs"""
    cs = d.cases(door, sg, scheme)
    assert set(FIXED[door]) == set(d.KINDS[door])
    for (kind, j), (item, want) in cs.items():
        assert type(want) is (bool if door in d.BOOL_DOORS else int)
        if FIXED[door][kind] is not None:
            assert want == FIXED[door][kind], (kind, j, want)
    assert {w for _, w in cs.values()} == d.STATUS_CLASSES[door]
    # an empty V fails except on the base item whose V is empty already
    if door == 'signcrypt':
        assert [cs['v_empty', j][1] for j in range(d.POOL)] == [d.msg_len(sg + scheme, j) == 0 for j in range(d.POOL)]
    for k in d.PREPARE_FAILS[door]:
        assert all(d.failed(cs[k, j][1]) for j in range(d.POOL)), k
    for k in d.NO_IDENTITY.get(door, ()):
        assert all(v is not None for j in range(d.POOL) for v in cs[k, j][0]), k
    if 'm' in d.COLS[door]:
        assert [len(cs[d.valid_kind(door), j][0][-1]) for j in range(d.POOL)] == [d.msg_len(sg + scheme, j) for j in range(d.POOL)]


def test_message_lengths():
    """the pools of a door take every length of MSG_LENS between them, the empty one included"""
    for door in ('sig_proof', 'signcrypt'):
        assert {d.msg_len(sg + scheme, j) for sg in (1, 2) for scheme in d.SCHEMES for j in range(d.POOL)} == set(d.MSG_LENS)
    assert {d.msg_len(t, j) for t in (1, 2, 3, 4) for j in range(d.POOL)} == set(d.MSG_LENS)          # core_verify and hashed
    for sg in (1, 2):
        assert [len(m) for m in d.hashed_messages(sg)] == [d.msg_len(sg + 2, j) for j in range(d.POOL)]


@pytest.mark.parametrize('sg', [1, 2])
@pytest.mark.parametrize('scheme', d.SCHEMES)
def test_sig_proof_kinds_are_what_they_say(sg, scheme):
    C = d.IMPLS[sg]
    S = C.sig_curve
    cs = d.cases('sig_proof', sg, scheme)
    other = d.SCHEMES[(d.SCHEMES.index(scheme) + 1) % 3]
    assert C.DST[other] != C.DST[scheme]
    for j in range(d.POOL):
        u, v, pk, y, msg = cs['valid', j][0]
        h = C.hash_to_point(msg, C.DST[scheme])
        assert 0 < y < c.R and all(0 <= cs[k, j][0][3] < c.R for k in d.KINDS['sig_proof'])          # canonical challenges
        assert cs['y_plus_1', j][0] == (u, v, pk, y + 1, msg)
        assert cs['msg_flip', j][0][4] != msg and len(cs['msg_flip', j][0][4]) == max(len(msg), 1)
        assert cs['other_key', j][0][2] != pk and cs['other_key', j][0][2] is not None
        # the right proof under another scheme's DST: it verifies there
        uo, vo, pko, yo, mo = cs['other_dst', j][0]
        assert (pko, yo, mo) == (pk, y, msg) and d.expected('sig_proof', sg, other, cs['other_dst', j][0]) == d.OK
        for kind, nones in (('u_inf', (0,)), ('v_inf', (1,)), ('pk_inf', (2,)), ('all_four', (0, 1, 2))):
            it = cs[kind, j][0]
            assert [k for k in range(3) if it[k] is None] == list(nones), kind
        assert cs['y_zero', j][0][3] == 0 and cs['all_four', j][0][3] == 0
        assert cs['y_one', j][0][3] == 1 and cs['y_r_minus_1', j][0][3] == c.R - 1
        ut, vt, _, yt, mt = cs['t_inf', j][0]
        assert ut is not None and vt is not None and mt == msg and S.add(ut, S.mul(h, yt)) is None      # T is the identity
        ud, vd, _, yd, md = cs['u_eq_yh', j][0]
        assert md == msg and ud == S.mul(h, yd) and ud is not None                                       # U + y H(m) doubles


@pytest.mark.parametrize('sg', [1, 2])
def test_core_doors_kinds_are_what_they_say(sg):
    C = d.IMPLS[sg]
    assert d.CORE_DST not in set(C.DST.values()) | {C.POP_DST}
    pop, core, hashed = d.cases('pop', sg), d.cases('core_verify', sg), d.cases('hashed', sg)
    for j in range(d.POOL):
        pk, proof = pop['valid', j][0]
        assert pop['other_proof', j][0][1] not in (proof, None)
        # a signature over the key bytes under the signing DST: Signature::verify accepts it, the proof-of-possession check does not
        pks, sig = pop['sign_dst', j][0]
        assert pks == pk and d._status_of(ref.verify, C, ref.POP, pk, sig, C.pk_to_bytes(pk)) == d.OK
        pk, sig, msg = core['valid', j][0]
        assert d._status_of(ref.core_verify, C, pk, core['scheme_dst', j][0][1], msg, C.DST[ref.BASIC]) == d.OK
        assert core['other_sig', j][0][1] not in (sig, None) and core['other_key', j][0][0] not in (pk, None)
        # the hashed door's points are the Basic scheme's hashes: its valid items are Signature::verify's
        pk, sig, h = hashed['valid', j][0]
        m = d.hashed_messages(sg)[j]
        assert h == C.hash_to_point(m, C.DST[ref.BASIC]) and d._status_of(ref.verify, C, ref.BASIC, pk, sig, m) == d.OK
        assert d._status_of(ref.verify, C, ref.BASIC, pk, sig, d.hashed_messages(sg)[(j + 1) % d.POOL]) == hashed['other_hash', j][1]
        pk, sig, h = hashed['h_inf', j][0]
        assert h is None and pk is not None and sig is not None
        assert (pk, sig) == hashed['valid', j][0][:2]


def test_signcrypt_and_pairing2_kinds_are_what_they_say():
    for sg in (1, 2):
        C = d.IMPLS[sg]
        for scheme in d.SCHEMES:
            cs = d.cases('signcrypt', sg, scheme)
            other = d.SCHEMES[(d.SCHEMES.index(scheme) + 1) % 3]
            for j in range(d.POOL):
                u, w, v = cs['valid', j][0]
                assert cs['v_empty', j][0] == (u, w, b'') and cs['v_flip', j][0][2] != v
                assert cs['other_w', j][0][1] not in (w, None)
                assert d.expected('signcrypt', sg, other, cs['other_dst', j][0]) is True
                assert [cs[k, j][0][:2].count(None) for k in ('u_inf', 'w_inf', 'both_inf')] == [1, 1, 2]
                assert cs['u_inf', j][0][0] is None and cs['w_inf', j][0][1] is None
    cs = d.cases('pairing2')
    trivial = lambda it: (it[0] is None or it[1] is None, it[2] is None or it[3] is None)  # noqa: E731
    for j in range(d.POOL):
        one = cs['one', j][0]
        for k, nm in enumerate(('g1a', 'g2a', 'g1b', 'g2b')):
            E, g = (c.E1, c.G1_GEN) if k % 2 == 0 else (c.E2, c.G2_GEN)
            off = cs['off_' + nm, j][0]
            assert off[k] == E.add(one[k], g) and off[:k] + off[k + 1:] == one[:k] + one[k + 1:]          # that scalar plus one
            inf = cs['inf_' + nm, j][0]
            assert inf[k] is None and inf.count(None) == 1 and sorted(trivial(inf)) == [False, True]      # exactly one pair trivial
        assert trivial(cs['both_trivial', j][0]) == (True, True) and cs['both_trivial', j][0].count(None) == 2
        assert cs['three_inf', j][0].count(None) == 3 and cs['four_inf', j][0].count(None) == 4
    assert {cs['both_trivial', j][0].index(None) for j in range(d.POOL)} == {0, 1}


def _decode(group, b, fmt):
    """a rendered point back to the oracle's affine form"""
    k = 1 if group == 1 else 2
    fe = (lambda o: util.fp_from_raw(b[o:o + 48])) if k == 1 else (lambda o: (util.fp_from_raw(b[o:o + 48]), util.fp_from_raw(b[o + 48:o + 96])))
    w = 48 * k
    if fmt == d.RAW_AFFINE:
        assert len(b) == 2 * w
        return None if b == bytes(2 * w) else (fe(0), fe(w))
    assert len(b) == 3 * w
    x, y, z = fe(0), fe(w), fe(2 * w)
    if z == (0 if k == 1 else (0, 0)):
        return None
    if k == 1:
        zi = c.fp_inv(z)
        return (x * zi * zi % c.P, y * zi * zi * zi % c.P)
    zi = c.f2_inv(z)
    zi2 = c.f2_sqr(zi)
    return (c.f2_mul(x, zi2), c.f2_mul(y, c.f2_mul(zi2, zi)))


@pytest.mark.parametrize('door,sg,scheme', [t for t in COMBOS if t[2] in (0, ref.POP)], ids=[i for t, i in zip(COMBOS, IDS) if t[2] in (0, ref.POP)])
def test_builder(door, sg, scheme):
    """the layouts: a failing item at item 0, at item n - 1 and on both sides of every 32-item boundary (so of every 64-item and of the
    last 128-item one), valid items around them; the expected vector is the pool's; every occurrence decodes to its pool item and
    no two occurrences of a point are byte-identical in RAW_PROJ"""
    cs = d.cases(door, sg, scheme)
    for n in d.SIZES[:10] + d.PLAN_SIZES:
        for fmt in (d.RAW_PROJ, d.RAW_AFFINE):
            if n > 129 and fmt == d.RAW_AFFINE:
                continue
            cols, want, names = d.build_batch(door, sg, scheme, n, 1, fmt=fmt)
            assert len(want) == len(names) == n and all(len(col) == n for col in cols) and len(cols) == len(d.COLS[door])
            assert want == [cs[nm][1] for nm in names]
            if n >= 4:
                sites = d.pinned_sites(n)
                assert {0, n - 1} <= set(sites) and all(b - 1 in sites and b in sites for b in range(32, n, 32))
                assert n < 129 or 128 * ((n - 1) // 128) in sites
                for s in sites:
                    assert d.failed(want[s]), (n, s, names[s])
                for b in range(32, n, 32):
                    assert not d.failed(want[b - 2]) and (b + 1 >= n - 1 or not d.failed(want[b + 1])), (n, b)
                assert not d.failed(want[1]) and (not d.failed(want[n - 2]) or (n - 2) % 32 in (0, 31))
            for k, t in enumerate(d.COLS[door]):
                if t in 'SK12':
                    group = {'S': sg, 'K': 3 - sg, '1': 1, '2': 2}[t]
                    for i in range(0, n, 7):
                        assert _decode(group, cols[k][i], fmt) == cs[names[i]][0][k], (n, i, names[i])
                    if fmt == d.RAW_PROJ:
                        finite = [cols[k][i] for i in range(n) if cs[names[i]][0][k] is not None]
                        assert len(set(finite)) == len(finite)
                else:
                    assert [cols[k][i] for i in range(n)] == [cs[nm][0][k] for nm in names]
    # every failing (kind, j) is placed somewhere in the largest layout; the one-item batches walk through every kind
    _, _, names = d.build_batch(door, sg, scheme, 1025, 0)
    assert set(d.fail_keys(door, sg, scheme)) <= set(names) and {k for k, _ in names} == set(d.KINDS[door])
    assert {d.build_batch(door, sg, scheme, 1, s)[2][0][0] for s in range(len(d.KINDS[door]))} == set(d.KINDS[door])
    for n in d.STALE_SIZES[:2]:
        assert not any(d.failed(x) for x in d.build_batch(door, sg, scheme, n, n % 7, 'all_valid')[1])
        assert all(d.failed(x) for x in d.build_batch(door, sg, scheme, n, n % 7, 'all_fail')[1])
        one = d.build_batch(door, sg, scheme, n, n % 7, 'all_but_one')
        assert [d.failed(x) for x in one[1]].count(False) == 1
        assert {k for k, _ in one[2]} <= set(d.PREPARE_FAILS[door]) | {d.valid_kind(door)}
