"""Worker for tests/test_gpu_keyset.py::test_single_set_indexed_large_path, and the cases of test_single_set_indexed: ONE set of five
positions of the key table, one of them twice, under the indexed secure call and under the by-value call on the gathered keys.  As a
program: the secure comparison for both signature groups in a fresh process (the BLSGPU_* knobs are read once, at library init).
Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDX = [3, 40, 9, 250, 3]


def cases(api, kc, sg, make):
    """{'good': [the set], 'tampered': [the set under the signature over another message]}; make: kc.multi_sets or kc.secure_sets"""
    (idx, sig, msg), (_, other, _) = make(api, sg, api.BASIC, kc.table(api, sg), None, idxs=[IDX, IDX])
    return {'good': [(idx, sig, msg)], 'tampered': [(idx, other, msg)]}


def secure_statuses(api, kc, sg, ks):
    """case -> [statuses of the indexed call, statuses of the by-value call]"""
    return {name: [api.verify_secure_indexed_batch(ks, api.BASIC, sets), api.verify_secure_batch(sg, api.BASIC, kc.gathered(api, ks, sets))]
            for name, sets in cases(api, kc, sg, kc.secure_sets).items()}


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    api.init()
    import keyset_cases as kc
    res = {}
    for sg in (1, 2):
        t = kc.table(api, sg)
        with api.KeySet.create(sg, t['blobs'], t['fmt']) as ks:
            res[str(sg)] = secure_statuses(api, kc, sg, ks)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
