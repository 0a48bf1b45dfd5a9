"""Hash-to-curve BEHIND expand_message_xmd on every kernel path, on chosen field elements (blsgpu_debug_map_to_curve: the shipped kernels
in their compile-time form that reads the uniform bytes from memory), against the oracle's integers.

The cases are the shared list of tests/h2c_cases.py (tests/test_h2c_cases.py proves it sound and runs it through the host build):
random bytes of every branch class, the edges of the 512-bit reduction in every block, u = 0, G1's u = +-sqrt(-1/11), u1 = u0 (the
addition of the two mapped points doubles), u1 = -u0 (the hash is the identity, Z = 0), G2's sgn0 fall-through, and the 16 elements of
Fp that SSWU sends to a pole of the 11-isogeny.  Every comparison is exact: RAW_PROJ (Jacobian) normalised to affine with Python
integers, the identity is Z = 0; Q is compared for the uncleared forms, H for the cleared ones; no case is left out on any path.

The (path, uncleared) pairs -- every one a launch of the library (csrc/blsgpu.hip), anything else is BLSGPU_E_ARG:
  G1 LANE 0            k_hash_to_g1(two_lanes = 0): run_hash_group beyond coop_max_items(); hash_to_g1(lane2 = -1) is also what
                       k_sign<1> and k_prepare_proof<1> call
  G1 LANE 1            hash_to_g1(lane2 = -1, no_clear): k_prepare<1> with one lane per item (BLSGPU_PREPARE_LANES = 1)
  G1 PAIR 0            k_hash_to_g1(two_lanes = 1): run_hash_group, 513 .. 4096 messages
  G1 PAIR 1            k_hash_to_g1(two_lanes = 1 | 2): run_hash_group(uncleared) beyond 1024 messages; k_prepare<1>(two_lanes | 2)
  G1 WIDE 0            k_hash_to_g1_wide: launch_hash_g1_small, 129 .. 512 messages
  G1 WIDE 1            k_hash_to_g1_wide(single_msg bit 1): run_hash_group(uncleared) up to 1024, run_verify_items 513 .. 1024
  G1 WIDE_REC 1        k_hash_to_g1_wide(out = null, rec): launch_hash_g1_small for the cut check, 129 .. 512 items
  G1 ENGINE 0          k_hash_to_g1_engine, program G1_HASH_TAIL: launch_hash_g1_small up to 128 messages
  G1 ENGINE 1          k_hash_to_g1_engine(out = null, rec), program G1_HASH_MAP: the cut check's record, up to 128 items; the door
                       converts the record's three engine values to RAW_PROJ (k_dbg_rec_g1_to_raw)
  G2 LANE 0            k_hash_to_g2(two_lanes = 0): hash_to_g2(lane2 = -1), what k_sign<2> and k_prepare_proof<2> call
  G2 PAIR 0            k_hash_to_g2(two_lanes = 1): run_hash_group beyond wide_max_items(); k_prepare<2>
  G2 PAIR 1            k_hash_to_g2(two_lanes = 3), Q as it stands between the two launches of the next row
  G2 PAIR_CLEAR_WIDE 0 k_hash_to_g2(two_lanes = 3) then k_g2_clear_wide: launch_hash_g2_small without scratch
  G2 ENGINE 0          k_hash_to_g2_engine (hash_g2_map_row, program G2_HASH_TAIL): launch_hash_g2_small up to 128 messages
  G2 MAPS_TAIL 0       k_hash_to_g2_maps then k_g2_hash_tail_wide: launch_hash_g2_small, 129 .. 512 messages
The cut check's record of the G2 engine forms (WREC_Q0) is a copy of the value-store words that `out` is converted from; it has no
door of its own.  The wave-per-message kernels are launched as the library launches them, one wave per workgroup.

Item counts put one item alone, fill a wave or workgroup, and spill one item into the next: one lane 1, 63, 64, 65; lane pair 1, 31,
32, 33, 65; wave per message 1, 4, 5, 129; workgroup per message 1, 2, 129.  Cases are taken from the list cyclically with a stride,
so doubling, identity and pole items sit beside regular ones in the same wave."""
import pytest

import h2c_cases as hc

pytestmark = pytest.mark.gpu

LANE, PAIR, WIDE, ENGINE, MAPS_TAIL, WIDE_REC, PAIR_CLEAR_WIDE = range(7)
NAMES = {LANE: 'LANE', PAIR: 'PAIR', WIDE: 'WIDE', ENGINE: 'ENGINE', MAPS_TAIL: 'MAPS_TAIL', WIDE_REC: 'WIDE_REC', PAIR_CLEAR_WIDE: 'PAIR_CLEAR_WIDE'}
FORMS = [(1, LANE, 0), (1, LANE, 1), (1, PAIR, 0), (1, PAIR, 1), (1, WIDE, 0), (1, WIDE, 1), (1, WIDE_REC, 1), (1, ENGINE, 0), (1, ENGINE, 1),
         (2, LANE, 0), (2, PAIR, 0), (2, PAIR, 1), (2, PAIR_CLEAR_WIDE, 0), (2, ENGINE, 0), (2, MAPS_TAIL, 0)]
IDS = ['G%d-%s-%s' % (g, NAMES[p], 'Q' if u else 'H') for g, p, u in FORMS]
COUNTS = {LANE: (1, 63, 64, 65), PAIR: (1, 31, 32, 33, 65), PAIR_CLEAR_WIDE: (1, 31, 32, 33, 65), WIDE: (1, 4, 5, 129), WIDE_REC: (1, 4, 5, 129),
          MAPS_TAIL: (1, 4, 5, 129), ENGINE: (1, 2, 129)}
STRIDE = 3                              # coprime to both list lengths (asserted below)

_whole = {}                             # (group, path, uncleared) -> the whole list's outputs, computed once


def run(api, form, cases):
    g, p, u = form
    outs = api.debug_map_to_curve(g, p, u, [cs['uniform'] for cs in cases])
    assert len(outs) == len(cases)
    return outs


def whole(api, form):
    if form not in _whole:
        _whole[form] = run(api, form, hc.build(form[0]))
    return _whole[form]


def what(form):
    return 'G%d %s,' % (form[0], NAMES[form[1]])


@pytest.mark.parametrize('form', FORMS, ids=IDS)
def test_whole_list(api, form):
    """every case of the group in one call"""
    for cs, o in zip(hc.build(form[0]), whole(api, form)):
        hc.check(cs, o, form[2], what(form))


@pytest.mark.parametrize('form', FORMS, ids=IDS)
def test_item_counts(api, form):
    lst = hc.build(form[0])
    assert len(lst) % STRIDE
    for k, n in enumerate(COUNTS[form[1]]):
        cases = hc.take(lst, n, 11 * k + 1, STRIDE)
        for cs, o in zip(cases, run(api, form, cases)):
            hc.check(cs, o, form[2], what(form) + ' %d items,' % n)


@pytest.mark.parametrize('form', FORMS, ids=IDS)
def test_both_positions(api, form):
    """the same cases shifted by one item -- the other lane pair of a quad, the other lane of a wave, the other block parity -- give
    identical output bytes: nothing may depend on where in the launch an item sits or on what its neighbour is"""
    lst = hc.build(form[0])
    sub = hc.take(lst, 23, 5, STRIDE)
    even = run(api, form, sub)
    odd = run(api, form, [lst[0]] + sub)[1:]
    for cs, a, b in zip(sub, even, odd):
        hc.check(cs, a, form[2], what(form))
        assert a == b, '%s case "%s": the result depends on the item\'s position' % (what(form), cs['name'])


@pytest.mark.parametrize('group', (1, 2))
def test_paths_agree(api, group):
    """all paths of a group agree with each other, point for point after normalisation (Q among the uncleared forms, H among the
    cleared ones), in addition to the comparison with the oracle"""
    lst = hc.build(group)
    for unc in (0, 1):
        forms = [f for f in FORMS if f[0] == group and f[2] == unc]
        pts = {f: [hc.normalise(group, o) for o in whole(api, f)] for f in forms}
        ref = forms[0]
        for f in forms[1:]:
            for cs, a, b in zip(lst, pts[ref], pts[f]):
                assert a == b, 'case "%s": %s and %s disagree' % (cs['name'], what(ref), what(f))


def test_unused_forms_are_refused(api, pkg):
    """an unknown path, and a (path, uncleared) pair that no launch of the library uses"""
    known = set(FORMS)
    u1, u2 = hc.build(1)[0]['uniform'], hc.build(2)[0]['uniform']
    for g in (0, 1, 2, 3):
        for p in range(-1, 8):
            for u in (0, 1, 2):
                if (g, p, u) not in known:
                    with pytest.raises(pkg.api.BlsGpuRuntimeError):
                        api.debug_map_to_curve(g, p, u, [u1 if g == 1 else u2])
