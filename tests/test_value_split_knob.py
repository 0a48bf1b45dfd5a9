"""BLSGPU_VALUE_SPLIT_MIN is a tuning row of the knob table, not an A/B switch: under BLSGPU_STRICT_ENV=1 blsgpu_init accepts it without
BLSGPU_AB_KNOBS and goes on to the device probe -- BLSGPU_E_NO_DEVICE on a machine without a GPU, success with one.  A value that is
no integer is refused as every row's is.  Child processes: the knobs are parsed once (tests/test_abi.py
test_strict_env_refuses_unknown_and_ungated_variables has the other rows)."""
import os
import subprocess
import sys

import util


def test_strict_env_knows_the_value_split_threshold():
    code = ("import ctypes, sys\n"
            "lib = ctypes.CDLL(%r)\n"
            "rc = lib.blsgpu_init(-1)\n"
            "buf = ctypes.create_string_buffer(512); lib.blsgpu_last_error(buf, 512)\n"
            "print(rc, buf.value.decode())\n") % os.path.join(util.ROOT, 'agora-blsful_amd', 'libblsgpu.so')
    import torch
    base = {k: v for k, v in os.environ.items() if not k.startswith('BLSGPU_')}

    def run(env):
        r = subprocess.run([sys.executable, '-c', code], env=dict(base, **env), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-1000:]
        rc, _, msg = r.stdout.strip().partition(' ')
        return int(rc), msg
    ok = (0,) if torch.cuda.is_available() else (-1,)           # BLSGPU_E_NO_DEVICE here, success on a GPU box
    for v in ('1', '0', '8192'):
        rc, msg = run({'BLSGPU_STRICT_ENV': '1', 'BLSGPU_VALUE_SPLIT_MIN': v})
        assert rc in ok, (v, rc, msg)
    rc, msg = run({'BLSGPU_STRICT_ENV': '1', 'BLSGPU_VALUE_SPLIT_MIN': 'many'})
    assert rc == -3 and 'BLSGPU_VALUE_SPLIT_MIN is not an integer' in msg
