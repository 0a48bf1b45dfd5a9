"""blsgpu_timecrypt_open_batch against tests/timecrypt_ref.py unseal, message for message and status for status: both impls, all three
schemes, groups of 0, 1, 2 and 5 items in one call with empty groups between, every message length at which a stage can go wrong,
crafted frames, every failure class and the pairs that pin their precedence, all four point formats, device-resident arguments, bad
offsets and a call that crosses the 4,096-item chunk.  The cases and everything expected of them come from tests/timecrypt_cases.py
(the oracle; tests/test_timecrypt_cases.py checks the list on the CPU, tests/test_hostsim_timecrypt.py runs the tail on the host).
Each test runs its calls in a fresh child process (tests/timecrypt_worker.py)."""
import pytest

import timecrypt_cases as tc
from test_gpu_pairing_value import run_worker

pytestmark = pytest.mark.gpu


def names_of(sg, fmt):
    wire = fmt in (tc.COMPRESSED, tc.LEGACY)
    return [it['name'] for g in tc.timelock_groups(sg) if wire or not g['sig_bad'] for it in g['items'] if wire or not it['u_bad']]


def diff(names, got, want):
    return [(i, names[i % len(names)], got[i], want[i]) for i in range(len(want)) if i >= len(got) or got[i] != want[i]][:8]


@pytest.mark.parametrize('sg', [1, 2])
def test_every_case_in_every_format(tmp_path, sg):
    """the whole case list as ONE call per format"""
    rendered = [tc.render_groups(sg, tc.timelock_groups(sg), fmt) for fmt in tc.FMTS]
    got = run_worker(tmp_path, 'cases%d' % sg, [{'op': 'timecrypt', 'sg': sg, 'groups': r[0], 'fmt': fmt} for r, fmt in zip(rendered, tc.FMTS)])
    assert len(got) == len(tc.FMTS)
    for (msgs, sts), (_, want_msgs, want_sts), fmt in zip(got, rendered, tc.FMTS):
        names = names_of(sg, fmt)
        assert sts == want_sts, (sg, fmt, diff(names, sts, want_sts))
        assert msgs == want_msgs, (sg, fmt, diff(names, msgs, want_msgs))
        assert all((m is not None) == (s == tc.OK) for m, s in zip(msgs, sts))


def test_device_pointers_and_bad_offsets(tmp_path):
    """every pointer as device memory (both impls; a failed item's range is (0, 0)); then offsets that do not start at 0 or that
    decrease: BLSGPU_E_ARG, and the same arguments with good offsets pass"""
    rendered = {sg: tc.render_groups(sg, tc.timelock_groups(sg), tc.COMPRESSED if sg == 1 else tc.RAW_PROJ, seed=3) for sg in (1, 2)}
    five = tc.render_groups(2, [g for g in tc.timelock_groups(2) if len(g['items']) == 5][:1], tc.RAW_PROJ)
    got = run_worker(tmp_path, 'device', [{'op': 'timecrypt_device', 'sg': sg, 'groups': rendered[sg][0], 'fmt': tc.COMPRESSED if sg == 1 else tc.RAW_PROJ}
                                          for sg in (1, 2)] + [{'op': 'timecrypt_bad_offsets', 'sg': 2, 'groups': five[0]}])
    for sg, (msgs, sts, rng) in zip((1, 2), got[:2]):
        assert sts == rendered[sg][2] and msgs == rendered[sg][1], (sg, diff(names_of(sg, tc.COMPRESSED if sg == 1 else tc.RAW_PROJ), sts, rendered[sg][2]))
        assert all(r == (0, 0) for r, s in zip(rng, sts) if s != tc.OK)
    rcs, sts = got[2]
    assert rcs == [-3, -3, -3, -3, 0] and sts == five[2] == [tc.OK] * 5


def test_chunk_boundary(tmp_path):
    """one call of 4,097 items, made by repeating the groups of the list: more than 400 groups, the last item alone in the second chunk"""
    n = 4097
    groups = tc.tiled_groups(1, n)
    api_groups, want_msgs, want_sts = tc.render_groups(1, groups, tc.RAW_AFFINE)
    (msgs, sts), = run_worker(tmp_path, 'chunk', [{'op': 'timecrypt', 'sg': 1, 'groups': api_groups, 'fmt': tc.RAW_AFFINE}])
    assert len(sts) == n and sts == want_sts and msgs == want_msgs
