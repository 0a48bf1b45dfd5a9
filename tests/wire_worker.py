"""Worker for tests/test_gpu_wire.py: the calls of a spec in a fresh process (the BLSGPU_* knobs are read once, when the library binds
its devices; the stale-pairs test needs one process with one context) -- prints one JSON line, a list with one status vector per
call.  It knows nothing of the oracle: the parent holds the expectations.
argv: spec.pickle, written by the parent: {'devices': k or 0, 'calls': [{'op': ..., ...}]}
  op 'wire'         blsgpu_verify_batch on host bytes            sg, scheme, fmt, pks, sigs, msgs
  op 'wire_device'  the same with every argument on the device   (and the status vector written there)
  op 'raw_valid'    n valid items signed on the device, verified as RAW_PROJ (leaves n valid pairs in the context)   sg, scheme, n"""
import ctypes
import json
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    spec = pickle.load(open(sys.argv[1], 'rb'))
    import torch
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    lib = api.load_library()
    if spec.get('devices'):
        nd = lib.blsgpu_init_devices(0)
        assert nd == spec['devices'] == lib.blsgpu_device_count(), nd
    else:
        api.init()
    res = []
    for cl in spec['calls']:
        if cl['op'] == 'wire':
            res.append(api.verify_batch(cl['sg'], cl['scheme'], cl['pks'], cl['sigs'], cl['msgs'], fmt=cl['fmt']))
        elif cl['op'] == 'raw_valid':
            n = cl['n']
            msgs = [b'stale pair %d' % i for i in range(n)]
            pks, sigs = api.sign_batch(cl['sg'], cl['scheme'], [0x77aa + 5 * i for i in range(n)], msgs)
            res.append(api.verify_batch(cl['sg'], cl['scheme'], pks, sigs, msgs))
        elif cl['op'] == 'wire_device':
            dev = torch.device('cuda', 0)
            T = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)  # noqa: E731
            P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
            n = len(cl['msgs'])
            offs = [0]
            for m in cl['msgs']:
                offs.append(offs[-1] + len(m))
            d_pks, d_sigs, d_msgs = T(b''.join(cl['pks'])), T(b''.join(cl['sigs'])), T(b''.join(cl['msgs']))
            d_offs = torch.tensor(offs, dtype=torch.int64, device=dev)
            d_st = torch.full((n,), -5, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            api._check(lib.blsgpu_verify_batch(cl['sg'], cl['scheme'], P(d_pks), P(d_sigs), P(d_msgs), P(d_offs), n, cl['fmt'], P(d_st)))
            res.append(d_st.cpu().tolist())
        else:
            raise ValueError(cl['op'])
    print(json.dumps(res))


if __name__ == '__main__':
    main()
