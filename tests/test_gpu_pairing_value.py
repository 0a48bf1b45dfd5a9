"""blsgpu_pairing_batch against tests/timecrypt_ref.py pairing_value, byte for byte and status for status: every format, one item to
more than a wave of workgroups, identities, undecodable wire points, device-resident arguments and a batch that crosses the 4,096-item
chunk of the host loop.  The items and everything expected of them come from tests/timecrypt_cases.py (the oracle;
tests/test_timecrypt_cases.py checks the list on the CPU).  Each test runs its calls in a fresh child process
(tests/timecrypt_worker.py)."""
import os
import pickle
import subprocess
import sys

import pytest

import timecrypt_cases as tc
import timecrypt_ref as tr
import util
from util import c, ref

pytestmark = pytest.mark.gpu


def run_worker(tmp_path, name, calls, timeout=300):
    """one attempt: a worker that dies by a signal or outlives its limit fails the test, and nothing further is started"""
    spec, out = str(tmp_path / (name + '.spec.pickle')), str(tmp_path / (name + '.out.pickle'))
    with open(spec, 'wb') as f:
        pickle.dump({'calls': calls}, f)
    keep = {k: v for k, v in os.environ.items() if not k.startswith('BLSGPU_') or k == 'BLSGPU_LIB'}
    r = subprocess.run([sys.executable, os.path.join(util.ROOT, 'tests', 'timecrypt_worker.py'), spec, out], env=keep, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, (name, r.returncode, r.stderr[-3000:])
    with open(out, 'rb') as f:
        return pickle.load(f)


def split(blob, n):
    assert len(blob) == tr.GT_BYTES * n
    return [blob[tr.GT_BYTES * i:tr.GT_BYTES * (i + 1)] for i in range(n)]


def diff(got, want):
    return [(i, got[i][:8].hex(), want[i][:8].hex()) for i in range(len(want)) if got[i] != want[i]][:8]


@pytest.mark.parametrize('fmt', tc.FMTS, ids=[tc.FMT_IDS[f] for f in tc.FMTS])
def test_sizes_and_special_items(tmp_path, fmt):
    """n = 1, 2, 3 and 65 (more than one block of the prepare kernel), then the special items: identities on either side and both,
    P and -P with one Q, and on the wire formats the pairs that do not decode"""
    batches = [tc.items(fmt, n, seed=n) for n in (1, 2, 3, 65)]
    names, g1s, g2s, want, st = tc.special_items(fmt)
    batches.append((g1s, g2s, want, st))
    got = run_worker(tmp_path, 'sizes', [{'op': 'pairing', 'g1s': b[0], 'g2s': b[1], 'fmt': fmt} for b in batches])
    assert len(got) == len(batches)
    for (blob, gst), b in zip(got, batches):
        rec = split(blob, len(b[2]))
        assert gst == b[3], (fmt, len(b[2]), gst)
        assert rec == b[2], (fmt, len(b[2]), diff(rec, b[2]))
    rec = split(got[-1][0], len(names))
    i, j = names.index('P'), names.index('-P')
    assert c.f12_mul(tr.gt_from_bytes(rec[i]), tr.gt_from_bytes(rec[j])) == c.F12_ONE      # multiplied on the host


def test_both_operand_orders_of_the_impls(tmp_path):
    """K = e(sig, u) as TimeCryptCiphertext::decrypt forms it: Bls12381G1Impl walks u (in G2), Bls12381G2Impl the signature; the G1
    member comes first in both"""
    g1s, g2s, want = [], [], []
    for sg in (1, 2):
        C = tr.IMPLS[sg]
        sk = ref.keygen_from_hash(bytes([40 + sg]) * 32)
        sig = C.sig_curve.mul(C.hash_to_point(b'round 7', C.DST[ref.BASIC]), sk)
        u = C.pk_curve.mul(C.pk_gen, 0x1234567 + sg)
        p1, p2 = (sig, u) if sg == 1 else (u, sig)
        g1s.append(util.g1_raw(p1))
        g2s.append(util.g2_raw(p2))
        want.append(tr.gt_bytes(tr.pairing_of(C, sig, u)))
    (blob, st), = run_worker(tmp_path, 'orders', [{'op': 'pairing', 'g1s': g1s, 'g2s': g2s, 'fmt': tc.RAW_PROJ}])
    assert st == [0, 0] and split(blob, 2) == want


def test_device_pointers_and_the_chunk_boundary(tmp_path):
    """every argument in device memory (65 items and the special ones), then one batch of 4,097 items -- the dozen distinct pairs
    repeated, the expected bytes tiled --, which crosses the chunk of the host loop"""
    b65 = tc.items(tc.RAW_PROJ, 65, seed=5)
    names, g1s, g2s, want, st = tc.special_items(tc.COMPRESSED)
    n = 4097
    one = tc.items(tc.RAW_AFFINE, len(tc.SCALARS))
    rep = lambda xs: [xs[i % len(xs)] for i in range(n)]  # noqa: E731
    got = run_worker(tmp_path, 'device', [
        {'op': 'pairing_device', 'g1s': b65[0], 'g2s': b65[1], 'fmt': tc.RAW_PROJ},
        {'op': 'pairing_device', 'g1s': g1s, 'g2s': g2s, 'fmt': tc.COMPRESSED},
        {'op': 'pairing', 'g1s': rep(one[0]), 'g2s': rep(one[1]), 'fmt': tc.RAW_AFFINE}])
    assert got[0][1] == b65[3] and split(got[0][0], 65) == b65[2]
    assert got[1][1] == st and split(got[1][0], len(names)) == want
    rec = split(got[2][0], n)
    assert got[2][1] == [0] * n and rec == rep(one[2]), diff(rec, rep(one[2]))
