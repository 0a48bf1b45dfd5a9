"""The model of tests/verify_shared_cases.py against the oracle: EVERY item of the case list, for both orientations and the three
schemes, verified on its own with its group's message (the C oracle's Signature::verify, pinned by the reference's known-answer
vectors in tests/test_oracle_c.py; one item of every kind once more by the Python oracle).  The list holds every
kind of item and group the calls distinguish, and the off-by-one pair would pass under the neighbouring group's message."""
import random

import pytest

import util
import verify_shared_cases as vc
from util import ref


@pytest.fixture(scope='module')
def bo():
    return util.load_c_oracle()


@pytest.mark.parametrize('sg,scheme', vc.COMBOS, ids=vc.COMBO_IDS)
def test_expected_statuses_are_the_oracles(bo, sg, scheme):
    rng = random.Random(10 * sg + scheme)
    for name, groups, expect in vc.batches(sg, scheme):
        raw = vc.raw_groups(sg, groups, rng)
        assert vc.oracle_statuses(bo, sg, scheme, raw) == expect, name
        assert len(expect) == sum(len(items) for _, items in groups)
    # the Python oracle on one item of every kind of the mixed batch
    _, groups, expect = vc.batches(sg, scheme)[2]
    flat = [(m, pk, sig) for m, items in groups for pk, sig in items]
    seen = set()
    for (m, pk, sig), want, name in zip(flat, expect, vc.names(scheme)):
        if name in seen:
            continue
        seen.add(name)
        try:
            ref.verify(vc.IMPLS[sg], scheme, pk, sig, m)
            got = vc.OK
        except ref.BlsError as e:
            got = vc.INVALID_SIGNATURE if e.kind == 'InvalidSignature' else vc.SIG_IDENTITY if 'signature is' in e.msg else vc.PK_IDENTITY
        assert got == want, name


@pytest.mark.parametrize('sg,scheme', vc.COMBOS, ids=vc.COMBO_IDS)
def test_off_by_one_items_pass_under_the_neighbour(bo, sg, scheme):
    """what makes the pair a test of the group lookup: each of the two verifies under the OTHER group's message"""
    _, groups, _ = vc.batches(sg, scheme)[2]
    raw = vc.raw_groups(sg, groups)
    by = {m: i for i, (m, _, _) in enumerate(raw)}
    a, b = raw[by[b'alpha']], raw[by[b'beta']]
    assert by[b'beta'] == by[b'alpha'] + 1
    assert bo.bo_verify(sg, scheme, a[1][-1], a[2][-1], b'beta', 4) == 0 and bo.bo_verify(sg, scheme, a[1][-1], a[2][-1], b'alpha', 5) == 1
    assert bo.bo_verify(sg, scheme, b[1][0], b[2][0], b'alpha', 5) == 0 and bo.bo_verify(sg, scheme, b[1][0], b[2][0], b'beta', 4) == 1


def test_kinds_present():
    for sg, scheme in vc.COMBOS:
        (n0, g0, e0), (n1, g1, e1), (_, groups, expect) = vc.batches(sg, scheme)
        assert g0 == [] and e0 == [] and all(not items for _, items in g1) and e1 == []
        sizes = [len(items) for _, items in groups]
        assert sizes[0] == 0 and sizes[-1] == 0 and 0 in sizes[1:-1] and 1 in sizes
        msgs = [m for m, _ in groups]
        assert b'' in msgs and msgs.count(b'same') == 2
        assert set(expect) == {vc.OK, vc.INVALID_SIGNATURE, vc.SIG_IDENTITY, vc.PK_IDENTITY}
        nm = vc.names(scheme)
        assert expect[nm.index('identity signature and identity key')] == vc.SIG_IDENTITY        # the signature wins
        assert expect[nm.index('identity key alone')] == vc.PK_IDENTITY
        assert expect[nm.index('tampered: signed by another key')] == vc.INVALID_SIGNATURE
        if scheme == ref.AUG:
            i = nm.index('own scalar, another key\'s prefix')
            assert expect[i:i + 2] == [vc.INVALID_SIGNATURE, vc.OK]


def test_strict_env_knows_the_knob():
    """BLSGPU_STRICT_ENV=1 with BLSGPU_SHARED_LINES_MIN set reaches the device probe (a fresh process: the knobs are read once);
    a value that is no integer is refused before it"""
    import os
    import subprocess
    import sys
    import torch
    code = ("import ctypes\n"
            "lib = ctypes.CDLL(%r)\n"
            "print(lib.blsgpu_init(-1), hasattr(lib, 'blsgpu_verify_shared_batch'), hasattr(lib, 'blsgpu_verify_shared_indexed_batch'))\n"
            ) % os.path.join(util.ROOT, 'agora-blsful_amd', 'libblsgpu.so')
    base = {k: v for k, v in os.environ.items() if not k.startswith('BLSGPU_')}

    def run(env):
        r = subprocess.run([sys.executable, '-c', code], env=dict(base, **env), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-1000:]
        rc, a, b = r.stdout.split()
        assert (a, b) == ('True', 'True')
        return int(rc)
    ok = 0 if torch.cuda.is_available() else -1           # BLSGPU_E_NO_DEVICE without a GPU
    assert run({'BLSGPU_STRICT_ENV': '1', 'BLSGPU_SHARED_LINES_MIN': '3'}) == ok
    assert run({'BLSGPU_STRICT_ENV': '1', 'BLSGPU_SHARED_LINES_MIN': '0'}) == ok
    assert run({'BLSGPU_STRICT_ENV': '1', 'BLSGPU_SHARED_LINES_MIN': 'many'}) == -3
