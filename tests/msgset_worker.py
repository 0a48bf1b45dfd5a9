"""Worker for tests/test_gpu_msgset.py: the message sets, key sets and steps of a spec in a fresh process (the BLSGPU_* knobs are read
once, when the library binds its devices) -- prints one JSON line {'steps': [result per step]}.  It knows nothing of the oracle: the
parent holds the expectations.
argv: spec.pickle, written by the parent:
    {'msgsets': {name: {'sg', 'scheme', 'msgs', 'lines'}},
     'keysets': {name: {'sg', 'keys', 'fmt', 'lines'}},
     'steps': [{'msgset': name, 'groups': [(msg_idx, pks, sigs)]}                     -- verify_msgset_batch
               | {'msgset': name, 'keyset': name, 'groups': [(msg_idx, idx, sigs)]}   -- verify_msgset_indexed_batch
               | {'msgset': name, 'update': (pos, msgs)} | {'msgset': name, 'append': msgs} | {'msgset': name, 'info': True}]}
A verify step gives {'st': flat statuses, 'launches': {kernel: count}}, an append the first new position, the others info()."""
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
    msets = {name: api.MessageSet.create(s['sg'], s['scheme'], s['msgs'], lines=s['lines']) for name, s in spec['msgsets'].items()}
    ksets = {name: api.KeySet.create(s['sg'], s['keys'], s['fmt'], lines=s['lines']) for name, s in spec.get('keysets', {}).items()}
    out = []
    seen = {k: v[1] for k, v in api.profile_read().items()}
    for step in spec['steps']:
        ms = msets[step['msgset']]
        if 'update' in step:
            ms.update(*step['update'])
            out.append(ms.info())
        elif 'append' in step:
            out.append(ms.append(step['append']))
        elif 'info' in step:
            out.append(ms.info())
        else:
            if 'keyset' in step:
                st = [s for g in api.verify_msgset_indexed_batch(ms, ksets[step['keyset']], step['groups']) for s in g]
            else:
                st = [s for g in api.verify_msgset_batch(ms, step['groups']) for s in g]
            now = {k: v[1] for k, v in api.profile_read().items()}
            out.append({'st': st, 'launches': {k: now[k] - seen.get(k, 0) for k in now if now[k] != seen.get(k, 0)}})
        seen = {k: v[1] for k, v in api.profile_read().items()}
    for s in list(msets.values()) + list(ksets.values()):
        s.close()
    print(json.dumps({'steps': out}))


if __name__ == '__main__':
    main()
