"""Worker for tests/test_gpu_pairing_doors.py: the calls of a spec in a fresh process (the BLSGPU_* knobs are read once, when the
library binds its devices; the stale-pairs test needs one process with one context) -- prints one JSON line, a list with one result
vector per call (statuses, or bools for the doors whose wrapper returns bools).  It knows nothing of the oracle: the parent holds
the expectations.
argv: spec.pickle, written by the parent: {'calls': [{'op': ..., 'door': ..., 'sg': ..., 'scheme': ..., 'fmt': ..., 'cols': [...], 'dst': ...}]}
  op 'host'     the door's entry point on host arguments (`call_door`, which the parent uses in-process as well)
  op 'device'   the same with every argument on the device (and the result vector written there)"""
import ctypes
import json
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINT_COLS = {'sig_proof': 3, 'pop': 2, 'signcrypt': 2, 'core_verify': 2, 'hashed': 3, 'pairing2': 4}    # the leading columns are points


def call_door(api, door, sg, scheme, cols, fmt=0, dst=b''):
    """one call of a door through its wrapper of agora-blsful_amd/api.py; cols as tests/pairing_door_cases.py COLS lists them"""
    if door == 'sig_proof':
        us, vs, pks, ys, msgs = cols
        return api.sig_proof_verify_batch(sg, scheme, us, vs, pks, ys, msgs, fmt=fmt)
    if door == 'pop':
        return api.pop_verify_batch(sg, cols[0], cols[1], fmt=fmt)
    if door == 'signcrypt':
        return api.signcrypt_valid_batch(sg, scheme, cols[0], cols[1], cols[2], fmt=fmt)
    if door == 'core_verify':
        return api.core_verify(sg, dst, cols[0], cols[1], cols[2], fmt=fmt)
    if door == 'hashed':
        assert fmt == 0
        return api.core_verify_hashed(sg, cols[0], cols[1], cols[2])
    assert door == 'pairing2', door
    return api.pairing2_check_batch(cols[0], cols[1], cols[2], cols[3], fmt=fmt)


def call_door_device(api, lib, door, sg, scheme, cols, fmt=0, dst=b''):
    """the same call with points, challenges, message blob, offsets and the result vector in device memory"""
    import torch
    dev = torch.device('cuda', 0)
    T = lambda b: torch.frombuffer(bytearray(b or b'\0'), dtype=torch.uint8).to(dev)  # noqa: E731
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    n = len(cols[0])
    d_st = torch.full((n,), -5, dtype=torch.int32, device=dev)

    def ragged(msgs):
        offs = [0]
        for m in msgs:
            offs.append(offs[-1] + len(m))
        return T(b''.join(msgs)), torch.tensor(offs, dtype=torch.int64, device=dev)
    pts = [T(b''.join(cols[k])) for k in range(POINT_COLS[door])]
    if door == 'sig_proof':
        d_ys = T(b''.join(int(y).to_bytes(32, 'little') for y in cols[3]))
        d_msgs, d_offs = ragged(cols[4])
        torch.cuda.synchronize()
        rc = lib.blsgpu_sig_proof_verify_batch(sg, scheme, P(pts[0]), P(pts[1]), P(pts[2]), P(d_ys), P(d_msgs), P(d_offs), n, fmt, P(d_st))
    elif door == 'pop':
        torch.cuda.synchronize()
        rc = lib.blsgpu_pop_verify_batch(sg, P(pts[0]), P(pts[1]), n, fmt, P(d_st))
    elif door == 'signcrypt':
        d_vs, d_offs = ragged(cols[2])
        torch.cuda.synchronize()
        rc = lib.blsgpu_signcrypt_valid_batch(sg, scheme, P(pts[0]), P(pts[1]), P(d_vs), P(d_offs), n, fmt, P(d_st))
    elif door == 'core_verify':
        d_msgs, d_offs = ragged(cols[2])
        torch.cuda.synchronize()
        rc = lib.blsgpu_core_verify(sg, api._ptr(dst), len(dst), P(pts[0]), P(pts[1]), P(d_msgs), P(d_offs), n, fmt, P(d_st))
    elif door == 'hashed':
        torch.cuda.synchronize()
        rc = lib.blsgpu_core_verify_hashed(sg, P(pts[0]), P(pts[1]), P(pts[2]), n, P(d_st))
    else:
        assert door == 'pairing2', door
        torch.cuda.synchronize()
        rc = lib.blsgpu_pairing2_check_batch(P(pts[0]), P(pts[1]), P(pts[2]), P(pts[3]), n, fmt, P(d_st))
    api._check(rc)
    st = d_st.cpu().tolist()
    if door == 'signcrypt':
        return [s == 0 for s in st]
    if door == 'pairing2':
        assert set(st) <= {0, 1}, sorted(set(st))
        return [bool(s) for s in st]
    return st


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    spec = pickle.load(open(sys.argv[1], 'rb'))
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    lib = api.load_library()
    api.init()
    res = []
    for cl in spec['calls']:
        args = (cl['door'], cl['sg'], cl['scheme'], cl['cols'], cl['fmt'], cl.get('dst', b''))
        if cl['op'] == 'host':
            res.append(call_door(api, *args))
        elif cl['op'] == 'device':
            res.append(call_door_device(api, lib, *args))
        else:
            raise ValueError(cl['op'])
    print(json.dumps(res))


if __name__ == '__main__':
    main()
