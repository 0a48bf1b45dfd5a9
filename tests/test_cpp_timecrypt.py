"""TimeCryptCiphertext of the C++ host mirror (include/blsful_hip.hpp) and its test program tests/cpp/timecrypt_test.cpp, built with
g++ against the C ABI only, as tests/test_cpp_pok_timestamp.py builds its program.  The ciphertexts are sealed by
tests/timecrypt_ref.py (the oracle) and handed over as "key hex" lines.

CPU: the program compiles, links against libblsgpu.so and FAILS LOUDLY without a device (no CPU path).
GPU: per orientation a round trip, an empty w, a wrong signature, a mismatched scheme and a length beyond the frame."""
import os
import subprocess

import pytest

import timecrypt_cases as tc
import timecrypt_ref as tr
import util
from oracle.py import blsful_ref as ref

ROOT = util.ROOT
LIBDIR = os.path.join(ROOT, 'agora-blsful_amd')


def build(tmp_path, with_cases):
    exe = str(tmp_path / 'timecrypt_test')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'),
                           os.path.join(ROOT, 'tests', 'cpp', 'timecrypt_test.cpp'), '-L', LIBDIR, '-lblsgpu', '-Wl,-rpath,' + LIBDIR, '-o', exe])
    lines = []
    for sg in ((1, 2) if with_cases else ()):
        C = tr.IMPLS[sg]
        scheme = (ref.POP, ref.BASIC)[sg - 1]
        sk = ref.keygen_from_hash(bytes([0x70 + sg]) * 32)
        pk = ref.public_key(C, sk)
        ident, msg, alpha = b'round 77', b'the C++ mirror opens this', bytes(range(32, 64))
        sig = C.sig_curve.mul(C.hash_to_point(ident, C.DST[scheme]), sk)
        bad_sig = C.sig_curve.mul(C.hash_to_point(b'round 78', C.DST[scheme]), sk)
        body = bytes(range(31))
        cts = {'ct_': tr.seal(C, pk, msg, ident, scheme, alpha), 'empty_': tr.seal_raw_frame(C, pk, ident, scheme, alpha, b''),
               'beyond_': tr.seal_raw_frame(C, pk, ident, scheme, alpha, bytes([32]) + body, message=body)}
        assert tr.unseal(C, cts['ct_'], sig, scheme) == (tr.OK, msg) and tr.unseal(C, cts['ct_'], bad_sig, scheme)[0] != tr.OK
        assert tr.unseal(C, cts['empty_'], sig, scheme) == (tr.OK, b'') and tr.unseal(C, cts['beyond_'], sig, scheme) == (tr.BAD_FRAME, None)
        pre = 'g%d_' % sg
        lines += [pre + 'msg ' + msg.hex(), pre + 'sig ' + tc.render_point(sg, sig, tc.RAW_PROJ, None).hex(),
                  pre + 'bad_sig ' + tc.render_point(sg, bad_sig, tc.RAW_PROJ, None).hex()]
        for k, (u, v, w, s) in cts.items():
            lines += [pre + k + 'u ' + tc.render_point(3 - sg, u, tc.RAW_PROJ, None).hex(), pre + k + 'v ' + v.hex(), pre + k + 'w ' + w.hex(),
                      pre + k + 'scheme %d' % s]
    kat = str(tmp_path / 'timecrypt_kats.txt')
    open(kat, 'w').write('\n'.join(lines) + '\n')
    return exe, kat


def test_cpp_timecrypt_builds_and_needs_a_device(pkg, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present: covered by test_cpp_timecrypt_on_gpu')
    exe, kat = build(tmp_path, False)
    p = subprocess.run([exe, kat], capture_output=True, text=True, timeout=120)
    assert p.returncode == 3 and 'no CPU fallback' in p.stdout, (p.returncode, p.stdout, p.stderr)


@pytest.mark.gpu
def test_cpp_timecrypt_on_gpu(pkg, tmp_path):
    exe, kat = build(tmp_path, True)
    p = subprocess.run([exe, kat], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and ' 0 failed' in p.stdout, (p.returncode, p.stdout[-3000:], p.stderr[-2000:])
