"""Worker for tests/test_gpu_keyset_lines.py: the key sets and calls of a spec in a fresh process (the BLSGPU_* knobs are read once,
when the library binds its devices) -- prints one JSON line {'sets': {name: info()}, 'calls': [{'st': flat statuses, 'launches':
{kernel: count}}]}.  It knows nothing of the oracle: the parent holds the expectations.
argv: spec.pickle, written by the parent:
    {'sets': {name: {'sg', 'keys', 'fmt', 'tables', 'lines'}},
     'calls': [{'set': name, 'scheme', 'idx', 'sigs', 'msgs'}                    -- verify_indexed_batch
               | {'set': name, 'scheme', 'groups': [(msg, idx, sigs)]}]}         -- verify_shared_indexed_batch"""
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
    sets = {name: api.KeySet.create(s['sg'], s['keys'], s['fmt'], tables=s['tables'], lines=s['lines']) for name, s in spec['sets'].items()}
    res = {'sets': {name: ks.info() for name, ks in sets.items()}, 'calls': []}
    seen = {k: v[1] for k, v in api.profile_read().items()}
    for cl in spec['calls']:
        ks = sets[cl['set']]
        if 'groups' in cl:
            st = [s for g in api.verify_shared_indexed_batch(ks, cl['scheme'], cl['groups']) for s in g]
        else:
            st = api.verify_indexed_batch(ks, cl['scheme'], cl['idx'], cl['sigs'], cl['msgs'])
        now = {k: v[1] for k, v in api.profile_read().items()}
        res['calls'].append({'st': st, 'launches': {k: now[k] - seen.get(k, 0) for k in now if now[k] != seen.get(k, 0)}})
        seen = now
    for ks in sets.values():
        ks.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
