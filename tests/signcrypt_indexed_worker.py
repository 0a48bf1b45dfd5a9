"""Worker for tests/test_gpu_signcrypt_indexed.py: the key sets and calls of a spec in a fresh process (the BLSGPU_* knobs are read
once, when the library binds its devices) -- prints one JSON line {'sets': {name: info()}, 'calls': [{'st': flat statuses, 'launches':
{kernel: count}}]}.  It knows nothing of the oracle: the parent holds the expectations.
argv: spec.pickle, written by the parent:
    {'sets': {name: {'sg', 'keys', 'fmt', 'lines'}},
     'calls': [{'set': name, 'scheme', 'cts': [(u, v, w)], 'shares': [[(position, share)]], 'fmt'}      -- the indexed call
               | {'sg', 'scheme', 'cts', 'pairs': [[(share, key share)]], 'fmt'}]}                        -- the by-value call"""
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
    sets = {name: api.KeySet.create(s['sg'], s['keys'], s['fmt'], lines=s['lines']) for name, s in spec['sets'].items()}
    res = {'sets': {name: ks.info() for name, ks in sets.items()}, 'calls': []}
    seen = {k: v[1] for k, v in api.profile_read().items()}
    for cl in spec['calls']:
        if 'set' in cl:
            st = api.signcrypt_share_verify_indexed_batch(cl['scheme'], sets[cl['set']], cl['cts'], cl['shares'], fmt=cl['fmt'])
        else:
            st = api.signcrypt_share_verify_batch(cl['sg'], cl['scheme'], cl['cts'], cl['pairs'], fmt=cl['fmt'])
        now = {k: v[1] for k, v in api.profile_read().items()}
        res['calls'].append({'st': [s for g in st for s in g], 'launches': {k: now[k] - seen.get(k, 0) for k in now if now[k] != seen.get(k, 0)}})
        seen = now
    for ks in sets.values():
        ks.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
