"""Worker for tests/test_gpu_secure_batch.py::test_every_plan_same_statuses: one blsgpu_verify_secure_batch call per sig_group
over a fixed mixed batch, in a fresh process (BLSGPU_SECURE_BATCH_MAX is read once, at library init).  Prints one JSON line:
{sig_group: statuses}."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    api.init()
    from secure_batch_cases import mixed_sets
    res = {}
    for sg in (1, 2):
        sets = mixed_sets(api, sg, api.BASIC, 70 + sg, big=100)
        res[sg] = api.verify_secure_batch(sg, api.BASIC, sets)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
