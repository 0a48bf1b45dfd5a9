"""Worker for tests/test_gpu_agg_msgset.py: the message sets, key sets and calls of a spec in a fresh process (the BLSGPU_* knobs are
read once, when the library binds its devices) -- prints one JSON line {'msgsets': {name: info()}, 'calls': [{'st': statuses,
'aux': [[a0, a1]], 'launches': {kernel: count}}]}.  It knows nothing of the oracle: the parent holds the expectations.
argv: spec.pickle, written by the parent:
    {'msgsets': {name: {'sg', 'scheme', 'msgs', 'lines'}},
     'keysets': {name: {'sg', 'keys', 'fmt'}},
     'calls': [{'msgset': name, 'sets': [(pks, msg_idx, sig)]}                      -- aggregate_verify_msgset_batch
               | {'msgset': name, 'keyset': name, 'sets': [(idx, msg_idx, sig)]}]}  -- aggregate_verify_msgset_indexed_batch"""
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
    ksets = {name: api.KeySet.create(s['sg'], s['keys'], s['fmt']) for name, s in spec.get('keysets', {}).items()}
    res = {'msgsets': {name: ms.info() for name, ms in msets.items()}, 'calls': []}
    seen = {k: v[1] for k, v in api.profile_read().items()}
    for cl in spec['calls']:
        if 'keyset' in cl:
            got = api.aggregate_verify_msgset_indexed_batch(msets[cl['msgset']], ksets[cl['keyset']], cl['sets'])
        else:
            got = api.aggregate_verify_msgset_batch(msets[cl['msgset']], cl['sets'])
        now = {k: v[1] for k, v in api.profile_read().items()}
        res['calls'].append({'st': [g[0] for g in got], 'aux': [list(g[1]) for g in got],
                             'launches': {k: now[k] - seen.get(k, 0) for k in now if now[k] != seen.get(k, 0)}})
        seen = now
    for s in list(msets.values()) + list(ksets.values()):
        s.close()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
