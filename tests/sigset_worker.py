"""Worker for tests/test_gpu_sigset.py: the calls of a spec in a fresh process (one library context from start to end) -- writes one
pickle, a list with one result per call.  It knows nothing of the oracle: the parent holds the expectations.
argv: spec.pickle result.pickle; spec = {'calls': [{'op': ..., ...}]}.  A call may carry 'set': {'sg', 'sigs', 'tags', 'fmt', 'lines',
optional 'append': [(sigs, tags, fmt)]} -- the set is created (and appended to) for the call and destroyed after it; every result
then starts with {'status': creation statuses, 'appended': [(first, statuses)], 'info': info(), 'kernels': {name: launches}}, the
kernels being those of the call alone (blsgpu_profile_get).
  op 'pairing'        api.pairing_batch(g1s, g2s, fmt) -> (gt bytes joined, statuses)
  op 'open'           api.timecrypt_open_batch(sg, groups, fmt, with_status=True) -> (messages or None, statuses)
  op 'sigset_pairing' api.pairing_sigset_batch(set, idx, points, fmt) -> (head, gt bytes joined, statuses)
  op 'sigset_pairing_device'  the same through TensorOps, every argument and result in device memory
  op 'sigset_open'    api.timecrypt_open_indexed_batch(set, items, fmt, with_status=True) -> (head, messages or None, statuses)
  op 'sigset_open_device'     the same through TensorOps -> (head, messages or None, statuses, ranges)
  op 'handles'        the C entry points on a destroyed id, a key set's id and a message set's id, and every kind's destroy, info,
                      update and append on the other two kinds' live ids -> the return codes"""
import ctypes
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev_ops(api):
    import torch
    dev = torch.device('cuda', 0)
    T = lambda b: torch.frombuffer(bytearray(b or b'\0'), dtype=torch.uint8).to(dev)  # noqa: E731
    U32 = lambda xs: torch.tensor([x - (1 << 32) if x >= 1 << 31 else x for x in xs] or [0], dtype=torch.int32, device=dev)  # noqa: E731
    I64 = lambda xs: torch.tensor(xs, dtype=torch.int64, device=dev)  # noqa: E731
    return api.TensorOps(dev), T, U32, I64


def pairing_device(api, s, idx, points, fmt):
    ops, T, U32, _ = dev_ops(api)
    out, st = ops.pairing_sigset_batch(s, U32(idx), T(b''.join(points)), len(points), fmt)
    return bytes(out.cpu().numpy().tobytes()), st.cpu().tolist()


def open_device(api, s, items, fmt):
    ops, T, U32, I64 = dev_ops(api)
    n = len(items)
    woffs = [0]
    for _, _, _, w, _ in items:
        woffs.append(woffs[-1] + len(w))
    ws = T(b''.join(w for _, _, _, w, _ in items))
    frames, rng, st = ops.timecrypt_open_indexed_batch(s, U32([k for k, *_ in items]), T(b''.join(u for _, u, _, _, _ in items)),
                                                       T(b''.join(v for _, _, v, _, _ in items)), ws if woffs[-1] else None, I64(woffs),
                                                       T(bytes(t for *_, t in items)), n, fmt)
    raw, rng, st = bytes(frames.cpu().numpy().tobytes()), rng.cpu().tolist(), st.cpu().tolist()
    return [raw[woffs[i] + rng[i][0]:woffs[i] + rng[i][0] + rng[i][1]] if st[i] == 0 else None for i in range(n)], st, [tuple(r) for r in rng]


def handles(api):
    """every entry point that takes a signature set's id, on a destroyed one, a key set's and a message set's; then destroy twice"""
    lib = api.load_library()
    g2 = bytes(192)
    s = api.SignatureSet.create(2, [g2], [0], api.FMT_RAW_AFFINE)
    dead = s.handle
    s.close()
    ks = api.KeySet.create(2, [bytes(96)], api.FMT_RAW_AFFINE)
    ms = api.MessageSet.create(2, api.BASIC, [b'm'])
    rcs = {}
    for name, h in (('destroyed', dead), ('key set', ks.handle), ('message set', ms.handle), ('zero', 0)):
        st = (ctypes.c_int32 * 1)()
        out = ctypes.create_string_buffer(576)
        rng = (ctypes.c_uint64 * 2)()
        first = ctypes.c_uint64(0)
        woffs = (ctypes.c_uint64 * 2)(0, 32)
        idx = (ctypes.c_uint32 * 1)(0)
        P = lambda x: ctypes.cast(x, ctypes.c_void_p)  # noqa: E731
        rcs[name] = [lib.blsgpu_sigset_info(h, None, None, None, None),
                     lib.blsgpu_sigset_append(h, api._ptr(g2), api._ptr(b'\0'), 1, api.FMT_RAW_AFFINE, None, ctypes.byref(first)),
                     lib.blsgpu_pairing_sigset_batch(h, P(idx), api._ptr(bytes(96)), 1, api.FMT_RAW_AFFINE, P(out), P(st)),
                     lib.blsgpu_timecrypt_open_indexed_batch(h, P(idx), api._ptr(bytes(96)), api._ptr(bytes(32)), api._ptr(bytes(32)), P(woffs), api._ptr(b'\0'), 1,
                                                             api.FMT_RAW_AFFINE, P(out), P(rng), P(st)),
                     lib.blsgpu_sigset_destroy(h)]
    # a key set's and a message set's own calls refuse a signature set's id
    s2 = api.SignatureSet.create(2, [g2], [0], api.FMT_RAW_AFFINE)
    rcs['as key set'] = [lib.blsgpu_keyset_destroy(s2.handle), lib.blsgpu_msgset_destroy(s2.handle)]
    # every kind's destroy, info, update (where it exists) and append, with the live ids of the other two kinds; then the three sets
    # are what they were
    P = lambda x: ctypes.cast(x, ctypes.c_void_p)  # noqa: E731
    pos, offs, first = (ctypes.c_uint32 * 1)(0), (ctypes.c_uint64 * 2)(0, 1), ctypes.c_uint64(0)
    before = [ks.info(), ms.info(), s2.info()]
    calls = {'key set': lambda h: [lib.blsgpu_keyset_destroy(h), lib.blsgpu_keyset_info(h, None, None, None, None),
                                   lib.blsgpu_keyset_update(h, P(pos), api._ptr(bytes(96)), 1, api.FMT_RAW_AFFINE, None),
                                   lib.blsgpu_keyset_append(h, api._ptr(bytes(96)), 1, api.FMT_RAW_AFFINE, None, ctypes.byref(first))],
             'message set': lambda h: [lib.blsgpu_msgset_destroy(h), lib.blsgpu_msgset_info(h, None, None, None, None, None),
                                       lib.blsgpu_msgset_update(h, P(pos), api._ptr(b'x'), P(offs), 1),
                                       lib.blsgpu_msgset_append(h, api._ptr(b'x'), P(offs), 1, ctypes.byref(first))],
             'signature set': lambda h: [lib.blsgpu_sigset_destroy(h), lib.blsgpu_sigset_info(h, None, None, None, None),
                                         lib.blsgpu_sigset_append(h, api._ptr(g2), api._ptr(b'\0'), 1, api.FMT_RAW_AFFINE, None, ctypes.byref(first))]}
    ids = {'key set': ks.handle, 'message set': ms.handle, 'signature set': s2.handle}
    rcs['wrong kind'] = {(kind, other): calls[kind](h) for kind in calls for other, h in ids.items() if other != kind}
    rcs['intact'] = [ks.info(), ms.info(), s2.info()] == before and [x['n'] for x in before] == [1, 1, 1]
    rcs['live'] = [lib.blsgpu_sigset_info(s2.handle, None, None, None, None), lib.blsgpu_sigset_destroy(s2.handle)]
    s2.handle = 0
    ks.close()
    ms.close()
    return rcs


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    spec = pickle.load(open(sys.argv[1], 'rb'))
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    api.init()
    res = []
    for cl in spec['calls']:
        s, head = None, None
        if 'set' in cl:
            d = cl['set']
            s = api.SignatureSet.create(d['sg'], d['sigs'], d['tags'], d['fmt'], lines=d['lines'])
            head = {'status': s.status, 'appended': [s.append(*a) for a in d.get('append', [])]}
            head['info'] = s.info()
            api.profile_enable(True)
        if cl['op'] == 'pairing':
            out, st = api.pairing_batch(cl['g1s'], cl['g2s'], cl['fmt'])
            r = (b''.join(out), st)
        elif cl['op'] == 'open':
            r = api.timecrypt_open_batch(cl['sg'], cl['groups'], cl['fmt'], with_status=True)
        elif cl['op'] == 'sigset_pairing':
            out, st = api.pairing_sigset_batch(s, cl['idx'], cl['points'], cl['fmt'])
            r = (b''.join(out), st)
        elif cl['op'] == 'sigset_pairing_device':
            r = pairing_device(api, s, cl['idx'], cl['points'], cl['fmt'])
        elif cl['op'] == 'sigset_open':
            r = api.timecrypt_open_indexed_batch(s, cl['items'], cl['fmt'], with_status=True)
        elif cl['op'] == 'sigset_open_device':
            r = open_device(api, s, cl['items'], cl['fmt'])
        elif cl['op'] == 'handles':
            r = (handles(api),)
        else:
            raise ValueError(cl['op'])
        if s is not None:
            head['kernels'] = {k: v[1] for k, v in api.profile_read().items()}
            api.profile_enable(False)
            s.close()
            r = (head,) + tuple(r)
        res.append(r)
    with open(sys.argv[2], 'wb') as f:
        pickle.dump(res, f)


if __name__ == '__main__':
    main()
