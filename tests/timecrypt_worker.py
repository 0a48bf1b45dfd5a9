"""Worker for tests/test_gpu_pairing_value.py and tests/test_gpu_timecrypt.py: the calls of a spec in a fresh process (one library
context from start to end) -- writes one pickle, a list with one result per call.  It knows nothing of the oracle: the parent holds the
expectations.
argv: spec.pickle result.pickle; spec = {'calls': [{'op': ..., ...}]}
  op 'pairing'          api.pairing_batch(g1s, g2s, fmt) on host arguments -> (gt bytes joined, statuses)
  op 'pairing_device'   the same with both point arrays, the 576-byte records and the statuses in device memory (TensorOps)
  op 'timecrypt'        api.timecrypt_open_batch(sg, groups, fmt, with_status=True) -> (messages or None, statuses)
  op 'timecrypt_device' the same with every argument and every result in device memory (TensorOps)
  op 'timecrypt_bad_offsets'  the C entry point on offsets that do not start at 0 or that decrease -> the return codes"""
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pairing_device(api, g1s, g2s, fmt):
    import torch
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    T = lambda b: torch.frombuffer(bytearray(b or b'\0'), dtype=torch.uint8).to(dev)  # noqa: E731
    out, st = ops.pairing_batch(T(b''.join(g1s)), T(b''.join(g2s)), len(g1s), fmt)
    return bytes(out.cpu().numpy().tobytes()), st.cpu().tolist()


def timecrypt_device(api, sg, groups, fmt):
    import torch
    dev = torch.device('cuda', 0)
    ops = api.TensorOps(dev)
    T = lambda b: torch.frombuffer(bytearray(b or b'\0'), dtype=torch.uint8).to(dev)  # noqa: E731
    I = lambda xs: torch.tensor(xs, dtype=torch.int64, device=dev)  # noqa: E731
    items = [ct for _, _, cts in groups for ct in cts]
    n = len(items)
    ioffs, woffs = [0], [0]
    for _, _, cts in groups:
        ioffs.append(ioffs[-1] + len(cts))
    for _, _, w, _ in items:
        woffs.append(woffs[-1] + len(w))
    ws = T(b''.join(w for _, _, w, _ in items))
    frames, rng, st = ops.timecrypt_open_batch(sg, T(b''.join(s for s, _, _ in groups)), T(bytes(t for _, t, _ in groups)), I(ioffs), len(groups),
                                               T(b''.join(u for u, _, _, _ in items)), T(b''.join(v for _, v, _, _ in items)),
                                               ws if woffs[-1] else None, I(woffs), T(bytes(t for _, _, _, t in items)), n, fmt)
    raw, rng, st = bytes(frames.cpu().numpy().tobytes()), rng.cpu().tolist(), st.cpu().tolist()
    return [raw[woffs[i] + rng[i][0]:woffs[i] + rng[i][0] + rng[i][1]] if st[i] == 0 else None for i in range(n)], st, [tuple(r) for r in rng]


def timecrypt_bad_offsets(api, sg, groups):
    """one valid single-group call's arguments with the offsets spoiled in turn: item_offsets from 1, decreasing; w_offsets from 1,
    decreasing"""
    import ctypes
    lib = api.load_library()
    (sig, tag, cts), = groups
    n = len(cts)
    assert n >= 2
    wlen = [len(w) for _, _, w, _ in cts]
    w_good = [sum(wlen[:i]) for i in range(n + 1)]
    U64 = lambda xs: (ctypes.c_uint64 * len(xs))(*xs)  # noqa: E731
    wblob = b''.join(w for _, _, w, _ in cts)
    frames = ctypes.create_string_buffer(len(wblob) + 64)
    rng = (ctypes.c_uint64 * (2 * n + 2))()
    st = (ctypes.c_int32 * (n + 1))()
    rcs = []
    for n_groups, ioffs, woffs in ((1, [1, n], w_good), (2, [0, n, n - 1], w_good), (1, [0, n], [1] + w_good[1:]),
                                   (1, [0, n], w_good[:1] + [w_good[2], w_good[1]] + w_good[3:]), (1, [0, n], w_good)):
        rcs.append(lib.blsgpu_timecrypt_open_batch(sg, api._ptr(sig * n_groups), api._ptr(bytes([tag]) * n_groups), ctypes.cast(U64(ioffs), ctypes.c_void_p), n_groups,
                                                   api._ptr(b''.join(u for u, _, _, _ in cts)), api._ptr(b''.join(v for _, v, _, _ in cts)), api._ptr(wblob),
                                                   ctypes.cast(U64(woffs), ctypes.c_void_p), api._ptr(bytes(t for _, _, _, t in cts)), 0,
                                                   ctypes.cast(frames, ctypes.c_void_p), ctypes.cast(rng, ctypes.c_void_p), ctypes.cast(st, ctypes.c_void_p)))
    return rcs, list(st)[:n]


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    spec = pickle.load(open(sys.argv[1], 'rb'))
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    api.init()
    res = []
    for cl in spec['calls']:
        if cl['op'] == 'pairing':
            out, st = api.pairing_batch(cl['g1s'], cl['g2s'], cl['fmt'])
            res.append((b''.join(out), st))
        elif cl['op'] == 'pairing_device':
            res.append(pairing_device(api, cl['g1s'], cl['g2s'], cl['fmt']))
        elif cl['op'] == 'timecrypt':
            res.append(api.timecrypt_open_batch(cl['sg'], cl['groups'], cl['fmt'], with_status=True))
        elif cl['op'] == 'timecrypt_device':
            res.append(timecrypt_device(api, cl['sg'], cl['groups'], cl['fmt']))
        elif cl['op'] == 'timecrypt_bad_offsets':
            res.append(timecrypt_bad_offsets(api, cl['sg'], cl['groups']))
        else:
            raise ValueError(cl['op'])
    with open(sys.argv[2], 'wb') as f:
        pickle.dump(res, f)


if __name__ == '__main__':
    main()
