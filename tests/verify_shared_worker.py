"""Worker for tests/test_gpu_verify_shared.py: the calls of a spec in a fresh process (the BLSGPU_* knobs are read once, when the
library binds its devices) -- prints one JSON line, a list with one {'st': flat statuses, 'launches': {kernel: count}} per call.
It knows nothing of the oracle: the parent holds the expectations.
argv: spec.pickle, written by the parent: {'calls': [{'sg': ..., 'scheme': ..., 'groups': [(msg, [pk], [sig])], 'fmt': ...}]}"""
import json
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    spec = pickle.load(open(sys.argv[1], 'rb'))
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    api.init()
    api.profile_enable(True)
    res = []
    seen = {}
    for cl in spec['calls']:
        st = api.verify_shared_batch(cl['sg'], cl['scheme'], cl['groups'], fmt=cl['fmt'])
        now = {k: v[1] for k, v in api.profile_read().items()}
        res.append({'st': [s for g in st for s in g], 'launches': {k: now[k] - seen.get(k, 0) for k in now if now[k] != seen.get(k, 0)}})
        seen = now
    print(json.dumps(res))


if __name__ == '__main__':
    main()
