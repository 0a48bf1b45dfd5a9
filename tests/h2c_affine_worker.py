"""Worker for tests/test_gpu_h2c_affine_iso.py: the calls of a spec in a fresh process (the BLSGPU_* knobs that choose the kernel
form are read once, when the library binds its device) -- prints one JSON line
    {'verify': statuses, 'aggregate': [[status, [aux0, aux1]], ...], 'hash': [RAW_PROJ hex, ...], 'launches': {kernel: count}}.
It knows nothing of the oracle: the parent holds the expectations.
argv: spec.pickle, written by the parent:
    {'scheme', 'pks', 'sigs', 'msgs'                      -- verify_batch, Bls12381G1Impl
     'aggregates': [(pks, msgs, sig)],                    -- aggregate_verify, one call each
     'hash_msgs', 'dst'}                                  -- hash_to_point into G1"""
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
    res = {'verify': api.verify_batch(1, spec['scheme'], spec['pks'], spec['sigs'], spec['msgs']), 'aggregate': []}
    for pks, msgs, sig in spec['aggregates']:
        st, aux = api.aggregate_verify(1, spec['scheme'], pks, msgs, sig)
        res['aggregate'].append([st, list(aux)])
    res['hash'] = [h.hex() for h in api.hash_to_point(1, spec['hash_msgs'], spec['dst'])]
    res['launches'] = {k: v[1] for k, v in api.profile_read().items() if v[1]}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
