"""Worker for tests/test_gpu_aggregate_batch.py: one call per sig_group over a fixed batch, in a fresh process (the BLSGPU_*
environment variables are read once, at library init).  `secure`: blsgpu_aggregate_secure_batch over mixed_sets with a 40-key set
(BLSGPU_SECURE_BATCH_MAX selects the plan); `sum`: blsgpu_sum_batch over ragged sets (BLSGPU_MULTI_STRIP selects the plan).
Prints one JSON line: {sig_group or group: [serialised points (hex), statuses]}."""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    api.init()
    from aggregate_batch_cases import mixed_sets, signed
    res = {}
    for g in (1, 2):
        if sys.argv[1] == 'secure':
            pts, sts = api.aggregate_secure_batch(g, mixed_sets(api, g, 70 + g, big=40))
        else:
            rng = random.Random(80 + g)
            sizes = [0, 1, 5, 64, 65, 9, 0, 130]
            keys = signed(api, 3 - g, [rng.randrange(1, 2 ** 200) for _ in range(sum(sizes))])[0]
            pts, sts = api.sum_batch(g, [keys[sum(sizes[:s]):sum(sizes[:s + 1])] for s in range(len(sizes))]), []
        res[g] = [[p.hex() for p in api.serialize(g, pts)], sts]
    print(json.dumps(res))


if __name__ == '__main__':
    main()
