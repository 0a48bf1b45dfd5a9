"""Worker for tests/test_gpu_value_split.py: the calls of a spec in a fresh process, under the BLSGPU_* variables its parent chose (the
knobs are parsed once, when the library binds its device) -- writes one pickle, a list with one result per call.  It knows nothing of
the oracle: the parent holds the expectations.  Every result is (kernels, ...): {name: launches} of that call alone
(blsgpu_profile_get), then what the call returned.  The device forms and the set handling are those of tests/timecrypt_worker.py and
tests/sigset_worker.py.
argv: spec.pickle result.pickle; spec = {'calls': [{'op': ..., ...}]}.  A call may carry 'set' as tests/sigset_worker.py describes it.
  op 'pairing' / 'pairing_device'   api.pairing_batch -> (gt bytes joined, statuses)
  op 'timecrypt'                    api.timecrypt_open_batch(..., with_status=True) -> (messages or None, statuses)
  op 'finalexp_value'               api.debug_finalexp_value(records, chunk, flags) -> (gt bytes joined,)
  op 'sigset_pairing'               api.pairing_sigset_batch -> (creation statuses, gt bytes joined, statuses)
  op 'sigset_open'                  api.timecrypt_open_indexed_batch(..., with_status=True) -> (creation statuses, messages or None, statuses)"""
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    spec = pickle.load(open(sys.argv[1], 'rb'))
    import __graft_entry__ as ge
    import timecrypt_worker
    api = ge.import_pkg().api
    api.init()
    res = []
    for cl in spec['calls']:
        s, head = None, ()
        if 'set' in cl:
            d = cl['set']
            s = api.SignatureSet.create(d['sg'], d['sigs'], d['tags'], d['fmt'], lines=d['lines'])
            for a in d.get('append', []):
                s.append(*a)
            head = (s.status,)
        api.profile_enable(True)
        if cl['op'] == 'pairing':
            out, st = api.pairing_batch(cl['g1s'], cl['g2s'], cl['fmt'])
            r = (b''.join(out), st)
        elif cl['op'] == 'pairing_device':
            r = timecrypt_worker.pairing_device(api, cl['g1s'], cl['g2s'], cl['fmt'])
        elif cl['op'] == 'timecrypt':
            r = api.timecrypt_open_batch(cl['sg'], cl['groups'], cl['fmt'], with_status=True)
        elif cl['op'] == 'finalexp_value':
            r = (b''.join(api.debug_finalexp_value([spec['records'][k] for k in cl['records']], cl['chunk'], cl['flags'])),)
        elif cl['op'] == 'sigset_pairing':
            out, st = api.pairing_sigset_batch(s, cl['idx'], cl['points'], cl['fmt'])
            r = (b''.join(out), st)
        elif cl['op'] == 'sigset_open':
            r = api.timecrypt_open_indexed_batch(s, cl['items'], cl['fmt'], with_status=True)
        else:
            raise ValueError(cl['op'])
        kernels = {k: v[1] for k, v in api.profile_read().items()}
        api.profile_enable(False)
        if s is not None:
            s.close()
        res.append((kernels,) + head + tuple(r))
    with open(sys.argv[2], 'wb') as f:
        pickle.dump(res, f)


if __name__ == '__main__':
    main()
