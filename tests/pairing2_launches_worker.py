"""Worker for tests/test_gpu_pairing2_launches.py: the sets and steps of a spec in a fresh process (the BLSGPU_* knobs are read once,
when the library binds its devices) -- prints one JSON line {name of the step: {'st': flat statuses, 'launches': {kernel: count}}}.
It knows nothing of the oracle or of the golden file: the parent holds both.
argv: spec.pickle, written by the parent:
    {'keysets': {name: {'sg', 'keys', 'fmt', 'lines'}},
     'msgsets': {name: {'sg', 'scheme', 'msgs', 'lines'}},
     'steps': [{'name', 'keyset', 'scheme', 'idx', 'sigs', 'msgs'}              -- verify_indexed_batch
               | {'name', 'sg', 'scheme', 'groups': [(msg, pks, sigs)]}         -- verify_shared_batch
               | {'name', 'msgset', 'groups': [(msg_idx, pks, sigs)]}           -- verify_msgset_batch
               | {'name', 'keyset', 'scheme', 'cts', 'shares'}                  -- signcrypt_share_verify_indexed_batch
               | {'name', 'door': a name of DOORS, ...}]}                       -- tests/test_gpu_item_keys_launches.py
A step with 'door' may give {'aux': [[aux0, aux1] per set]} next to 'st' (the aggregate doors)."""
import json
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def flat(rows):
    return {'st': [s for g in rows for s in g]}


def with_aux(rows):
    return {'st': [s for s, _ in rows], 'aux': [list(a) for _, a in rows]}


# door -> fn(api, key sets, message sets, step): {'st': flat statuses[, 'aux']}
DOORS = {
    'verify_indexed': lambda api, ks, ms, s: {'st': api.verify_indexed_batch(ks[s['keyset']], s['scheme'], s['idx'], s['sigs'], s['msgs'], fmt=s['fmt'])},
    'verify_shared_indexed': lambda api, ks, ms, s: flat(api.verify_shared_indexed_batch(ks[s['keyset']], s['scheme'], s['groups'])),
    'verify_msgset_indexed': lambda api, ks, ms, s: flat(api.verify_msgset_indexed_batch(ms[s['msgset']], ks[s['keyset']], s['groups'])),
    'signcrypt_share_verify': lambda api, ks, ms, s: flat(api.signcrypt_share_verify_batch(s['sg'], s['scheme'], s['cts'], s['pairs'])),
    'aggregate_verify_indexed': lambda api, ks, ms, s: with_aux(api.aggregate_verify_indexed_batch(ks[s['keyset']], s['scheme'], s['sets'])),
    'aggregate_verify_msgset_indexed': lambda api, ks, ms, s: with_aux(api.aggregate_verify_msgset_indexed_batch(ms[s['msgset']], ks[s['keyset']], s['sets'])),
}


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    spec = pickle.load(open(sys.argv[1], 'rb'))
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    api.init()
    api.profile_enable(True)
    ksets = {name: api.KeySet.create(s['sg'], s['keys'], s['fmt'], lines=s['lines']) for name, s in spec['keysets'].items()}
    msets = {name: api.MessageSet.create(s['sg'], s['scheme'], s['msgs'], lines=s['lines']) for name, s in spec['msgsets'].items()}
    out = {}
    seen = {k: v[1] for k, v in api.profile_read().items()}
    for step in spec['steps']:
        more = {}
        if 'door' in step:
            more = DOORS[step['door']](api, ksets, msets, step)
            st = more.pop('st')
        elif 'cts' in step:
            st = [s for g in api.signcrypt_share_verify_indexed_batch(step['scheme'], ksets[step['keyset']], step['cts'], step['shares']) for s in g]
        elif 'msgset' in step:
            st = [s for g in api.verify_msgset_batch(msets[step['msgset']], step['groups']) for s in g]
        elif 'groups' in step:
            st = [s for g in api.verify_shared_batch(step['sg'], step['scheme'], step['groups']) for s in g]
        else:
            st = api.verify_indexed_batch(ksets[step['keyset']], step['scheme'], step['idx'], step['sigs'], step['msgs'])
        now = {k: v[1] for k, v in api.profile_read().items()}
        out[step['name']] = dict(more, st=st, launches={k: now[k] - seen.get(k, 0) for k in now if now[k] != seen.get(k, 0)})
        seen = now
    for s in list(ksets.values()) + list(msets.values()):
        s.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
