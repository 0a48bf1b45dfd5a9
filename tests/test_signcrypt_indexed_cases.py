"""The case list of tests/signcrypt_indexed_cases.py on the CPU: every class of the indexed share check is present for both impls, the
table's invalid entry really fails decoding, and a handful of the expected statuses are the oracle's pairings
(oracle/py/blsful_ref.py signcrypt_verify_share with the key the position names) -- at most 24 pairing products, counted.  The knob of
the call's table plan is known to the library's strict environment check (a fresh process each, no device needed to refuse)."""
import os
import subprocess
import sys

import pytest

import signcrypt_cases as sc
import signcrypt_indexed_cases as ic
import test_signcrypt_cases as tsc
import util
from util import c, ref

MAX_PRODUCTS = 24


@pytest.mark.parametrize('sg', [1, 2])
def test_every_class_is_present(sg):
    cl = ic.cases(sg)
    for k in ic.CLASSES:
        assert any(k in x.classes for x in cl), k
    flat = [(x, pos, a, st) for x in cl for (pos, a), st in zip(x.shares, x.expected())]
    assert {st for _, _, _, st in flat} == {ic.OK, ic.INVALID_DECRYPTION_SHARE, ic.E_ARG, ic.BAD_ENCODING}
    t = ic.table(sg)
    assert len(t['ks']) == ic.N and t['ks'][ic.IDENT] == 0 and t['ks'][ic.BAD] is None
    # what each class promises
    by = lambda k: [x for x in cl if k in x.classes]
    assert any(ic.OK in x.expected() for x in by('valid'))
    assert all(x.expected().count(ic.INVALID_DECRYPTION_SHARE) == 1 and x.expected().count(ic.OK) == 2 for x in by('tampered share'))
    swapped = next(x for x in cl if x.name == 'right shares, two positions swapped')
    assert swapped.expected() == [ic.INVALID_DECRYPTION_SHARE, ic.INVALID_DECRYPTION_SHARE, ic.OK]
    assert any(a % ic.R == 0 and pos < ic.N and st == ic.INVALID_DECRYPTION_SHARE for _, pos, a, st in flat)                 # identity share
    assert any(pos == ic.IDENT and a % ic.R and st == ic.INVALID_DECRYPTION_SHARE for _, pos, a, st in flat)                 # identity entry
    assert all(st == ic.BAD_ENCODING for _, pos, _, st in flat if pos == ic.BAD) and any(pos == ic.BAD for _, pos, _, _ in flat)
    assert all(st == ic.E_ARG for _, pos, _, st in flat if pos >= ic.N) and {pos for _, pos, _, _ in flat if pos >= ic.N} == {ic.N, 2 ** 32 - 1}
    assert all(x.cs.w is None and set(x.expected()) <= {ic.INVALID_DECRYPTION_SHARE, ic.BAD_ENCODING, ic.E_ARG} for x in by('identity w'))
    assert all(x.call_scheme != x.cs.scheme and set(x.expected()) == {ic.INVALID_DECRYPTION_SHARE} for x in by('wrong-scheme DST'))
    assert all(x.shares == [] for x in by('0 shares'))
    rep = by('repeated position')[0]
    assert rep.expected() == [ic.OK] * 4 and len({pos for pos, _ in rep.shares}) == 2
    assert all(x.cs.v == b'' and ic.OK in x.expected() for x in by('empty v'))
    assert {x.call_scheme for x in cl} == {ref.BASIC, ref.AUG, ref.POP}
    # the list of signcrypt_cases is all here, except the one case whose seventeen key shares are not committee members
    names = {x.cs.name for x in cl}
    assert {cs.name for cs in sc.cases(sg)} - names == set()


@pytest.mark.parametrize('sg', [1, 2])
def test_the_invalid_entry_fails_decoding_and_the_others_decode(sg):
    t = ic.table(sg)
    dec = c.g2_decompress if sg == 1 else c.g1_decompress
    for k, b in zip(t['ks'], t['blobs']):
        if k is None:
            with pytest.raises(c.DecodeError):
                dec(b)
        else:
            assert dec(b) == sc.pk_point(sg, k)


def test_a_handful_of_statuses_are_the_oracles_pairings():
    with tsc.Counter() as cnt:
        picked = set()
        for sg in (1, 2):
            C = sc.IMPLS[sg]
            t = ic.table(sg)
            want = ['tampered share', 'right shares, two positions swapped', 'a share under the identity entry', 'a repeated position',
                    'an Aug ciphertext under the Basic DST', 'identity w' if sg == 1 else 'crafted frame: empty v']
            for x in ic.cases(sg):
                if x.name not in want:
                    continue
                for (pos, a), st in list(zip(x.shares, x.expected()))[:2]:
                    assert st in (ic.OK, ic.INVALID_DECRYPTION_SHARE)
                    got = ref.signcrypt_verify_share(C, sc.pk_point(sg, a), sc.pk_point(sg, t['ks'][pos]), x.cs.u, x.cs.v, x.cs.w, C.DST[x.call_scheme])
                    assert got == (st == ic.OK), (sg, x.name, pos)
                    picked.add((x.name, st))
        assert len(picked) >= 8 and {st for _, st in picked} == {ic.OK, ic.INVALID_DECRYPTION_SHARE}
    assert 0 < cnt.n <= MAX_PRODUCTS, cnt.n


def test_strict_env_knows_the_knob():
    """BLSGPU_STRICT_ENV=1 with BLSGPU_SIGNCRYPT_LINES_MIN set reaches the device probe (a fresh process: the knobs are read once); a
    value that is no integer is refused before it, and so is a misspelt name"""
    import torch
    code = ("import ctypes\n"
            "lib = ctypes.CDLL(%r)\n"
            "print(lib.blsgpu_init(-1), hasattr(lib, 'blsgpu_signcrypt_share_verify_indexed_batch'), hasattr(lib, 'blsgpu_debug_tables2'))\n"
            ) % os.path.join(util.ROOT, 'agora-blsful_amd', 'libblsgpu.so')
    base = {k: v for k, v in os.environ.items() if not k.startswith('BLSGPU_')}

    def run(env):
        r = subprocess.run([sys.executable, '-c', code], env=dict(base, **env), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-1000:]
        rc, a, b = r.stdout.split()
        assert (a, b) == ('True', 'True')
        return int(rc)
    ok = 0 if torch.cuda.is_available() else -1           # BLSGPU_E_NO_DEVICE without a GPU
    assert run({'BLSGPU_STRICT_ENV': '1', 'BLSGPU_SIGNCRYPT_LINES_MIN': '4'}) == ok
    assert run({'BLSGPU_STRICT_ENV': '1', 'BLSGPU_SIGNCRYPT_LINES_MIN': '0'}) == ok
    assert run({'BLSGPU_STRICT_ENV': '1', 'BLSGPU_SIGNCRYPT_LINES_MIN': 'many'}) == -3
    assert run({'BLSGPU_STRICT_ENV': '1', 'BLSGPU_SIGNCRYPT_LINE_MIN': '4'}) == -3
