"""The case list of tests/h2c_cases.py is sound, and the one-lane map code of csrc/h2c.cuh compiled for the host (tests/hostsim
hs_map_to_curve: hash_to_g1_map / hash_to_g2_map, what the door blsgpu_debug_map_to_curve runs on the device) maps every case to the
oracle's points, exactly -- with the bound tracker on, so every case is also proved to lie inside the contracts of fp_set_words / fp_mul."""
import ctypes

import pytest

import h2c_cases as hc
from oracle.py import bls381 as c

FAMILIES = {1: ('random', 'edge', 'zero', 'tv2', 'eqopp', 'pole'), 2: ('random', 'edge', 'zero', 'eqopp', 'sgn0')}


@pytest.mark.parametrize('group', (1, 2))
def test_list_is_sound(group):
    lst = hc.build(group)
    assert lst is hc.build(group)                                  # built once, left unchanged
    by = {}
    for cs in lst:
        by.setdefault(cs['family'], []).append(cs)
        assert len(cs['uniform']) == 128 * group
        assert (c.E1 if group == 1 else c.E2).on_curve(cs['Q']) and (c.E1 if group == 1 else c.E2).on_curve(cs['H'])
    assert set(by) == set(FAMILIES[group]) and all(by[f] for f in by)
    assert len(by['random']) >= 32
    assert len({cs['name'] for cs in lst}) == len(lst)
    # consecutive cases differ, the wrap-around included: both their bytes and their field elements
    for i, cs in enumerate(lst):
        nxt = lst[(i + 1) % len(lst)]
        assert cs['uniform'] != nxt['uniform'] and cs['u'] != nxt['u'], cs['name']
    # every branch class among the random cases, in both positions (build() asserts it too)
    seen = {(pos, cl) for cs in by['random'] for pos, cl in enumerate(cs['classes'])}
    assert seen == {(pos, (sq, fl)) for pos in (0, 1) for sq in (False, True) for fl in (False, True)}
    # the exceptional classes really are what their names say
    zero = 0 if group == 1 else (0, 0)
    assert sum(cs['u'][0] == zero for cs in by['zero']) >= 6 and sum(cs['u'][1] == zero for cs in by['zero']) >= 6
    both = [cs for cs in by['zero'] if cs['u'] == (zero, zero)]
    mp = c.map_to_curve_g1 if group == 1 else c.map_to_curve_g2
    E = c.E1 if group == 1 else c.E2
    assert len(both) == 3 and all(cs['Q'] == E.dbl(mp(zero)) and cs['Q'] is not None for cs in both)
    eq = [cs for cs in by['eqopp'] if cs['u'][0] == cs['u'][1]]
    opp = [cs for cs in by['eqopp'] if cs['u'][0] != cs['u'][1]]
    assert len(eq) == 8 and len(opp) == 8
    assert all(cs['Q'] == E.dbl(mp(cs['u'][0])) for cs in eq)
    assert sum(cs['uniform'][:64 * group] != cs['uniform'][64 * group:] for cs in eq) == 4         # the same element in other bytes
    assert all(cs['Q'] is None and cs['H'] is None for cs in opp)
    assert all(mp((-cs['u'][0]) % c.P if group == 1 else c.f2_neg(cs['u'][0])) == E.neg(mp(cs['u'][0])) for cs in opp)


def test_g1_exceptional_inputs():
    lst = hc.build(1)
    poles = [cs for cs in lst if cs['family'] == 'pole']
    single = [cs for cs in poles if 'position' in cs['name']]
    assert len(single) == 32 and len({cs['u'][0] for cs in single if 'position 0' in cs['name']}) == 16
    for cs in single:
        k = 0 if 'position 0' in cs['name'] else 1
        assert c.map_to_curve_g1(cs['u'][k]) is None and c.map_to_curve_g1(cs['u'][1 - k]) is not None
        assert cs['Q'] == c.map_to_curve_g1(cs['u'][1 - k]) and cs['H'] == c.E1.mul(cs['Q'], c.H_EFF_G1) and cs['H'] is not None
    assert all(cs['Q'] is None and cs['H'] is None for cs in poles if 'poles' in cs['name'])
    s, ns = hc.g1_tv2_zero_inputs()
    tv2 = [cs for cs in lst if cs['family'] == 'tv2']
    assert {u for cs in tv2 for u in cs['u']} >= {s, ns}
    assert all(hc.classify(1, u) is None for u in (0, s, ns))


def test_g2_sgn0_inputs():
    for cs in hc.build(2):
        if cs['family'] == 'sgn0':
            u = cs['u'][0] if 'u0' in cs['name'] else cs['u'][1]
            assert (u[0] == 0) != (u[1] == 0)
            if '(0, odd)' in cs['name']:
                assert c._sgn0_f2(u) == 1 and u[0] == 0
            if '(0, even)' in cs['name']:
                assert c._sgn0_f2(u) == 0 and u[0] == 0


def test_reduction_edges_cover_every_block():
    for group in (1, 2):
        edge = [cs for cs in hc.build(group) if cs['family'] == 'edge']
        assert len(edge) == len(hc.EDGES) * 2 * group
        for nm, v in hc.EDGES:
            for pos in range(2 * group):
                assert any(cs['uniform'][64 * pos:64 * pos + 64] == v.to_bytes(64, 'big') for cs in edge), (nm, pos)


@pytest.mark.parametrize('uncleared', (0, 1))
@pytest.mark.parametrize('group', (1, 2))
def test_host_build_maps_every_case(hs, group, uncleared):
    """hash_to_g1_map / hash_to_g2_map on the host, cleared and uncleared, against the oracle: exact after normalisation"""
    hs.hs_map_to_curve.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p]
    hs.hs_map_to_curve.restype = None
    for cs in hc.build(group):
        out = ctypes.create_string_buffer(144 * group)
        hs.hs_map_to_curve(group, cs['uniform'], uncleared, out)
        hc.check(cs, out.raw, uncleared, 'host build,')
