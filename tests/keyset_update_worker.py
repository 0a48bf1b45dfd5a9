"""Worker for tests/test_gpu_keyset_update.py: the key sets and steps of a spec in a fresh process (the BLSGPU_* knobs are read once,
when the library binds its devices) -- prints one JSON line {'steps': [result of every step]}.  It knows nothing of the oracle: the
parent holds the expectations.
argv: spec.pickle, written by the parent:
    {'sets': {name: {'sg', 'keys', 'fmt', 'tables', 'lines'}},
     'steps': [{'op': 'update', 'set', 'pos', 'keys', 'fmt'}          -> {'st', 'launches'}
               | {'op': 'append', 'set', 'keys', 'fmt'}               -> {'first', 'st', 'launches'}
               | {'op': 'verify', 'set', 'scheme', 'idx', 'sigs', 'msgs'}   -> {'st', 'launches'}     (verify_indexed_batch)
               | {'op': 'info', 'set'}                                -> info()
               | {'op': 'get', 'set', 'idx'}                          -> {'keys': hex of the Modern bytes, 'st'}]}"""
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
    out = []
    seen = {k: v[1] for k, v in api.profile_read().items()}
    for step in spec['steps']:
        ks = sets[step['set']]
        if step['op'] == 'update':
            res = {'st': ks.update(step['pos'], step['keys'], step['fmt'])}
        elif step['op'] == 'append':
            first, st = ks.append(step['keys'], step['fmt'])
            res = {'first': first, 'st': st}
        elif step['op'] == 'verify':
            res = {'st': api.verify_indexed_batch(ks, step['scheme'], step['idx'], step['sigs'], step['msgs'])}
        elif step['op'] == 'get':
            keys, st = ks.get(step['idx'], api.FMT_COMPRESSED)
            res = {'keys': b''.join(keys).hex(), 'st': st}
        else:
            res = ks.info()
        now = {k: v[1] for k, v in api.profile_read().items()}
        if step['op'] in ('update', 'append', 'verify'):
            res['launches'] = {k: now[k] - seen.get(k, 0) for k in now if now[k] != seen.get(k, 0)}
        seen = now
        out.append(res)
    for ks in sets.values():
        ks.close()
    print(json.dumps({'steps': out}))


if __name__ == '__main__':
    main()
