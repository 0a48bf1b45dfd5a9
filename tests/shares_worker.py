"""Worker for tests/test_gpu_shares.py::test_every_plan_same_bytes: one blsgpu_combine_shares call per group over ragged sets (and two
failing ones) built from a fixed seed, in a fresh process (BLSGPU_SHARES_MSM_MIN is read once, at library init).  Prints one JSON
line: {group: [statuses, hex of every output point]}."""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SIZES = [0, 1, 2, 3, 17, 63, 64, 65, 240, 400, 1000]


def main():
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    from test_gpu_shares import R, distinct_ids, points
    res = {}
    for group in (1, 2):
        rng = random.Random(31 + group)
        sets = []
        for t in SIZES + [5, 70]:
            ids = distinct_ids(rng, t)
            ks = [rng.randrange(R) for _ in range(t)]
            if t == 5:
                ids[4] = ids[0]           # duplicate
            if t == 70:
                ids[10] = 0               # zero identifier
            sets.append(list(zip(ids, points(api, group, ks), [None] * t)))
        out, st = api.combine_shares(group, sets)
        res[group] = [st, [o.hex() for o in out]]
    print(json.dumps(res))


if __name__ == '__main__':
    main()
