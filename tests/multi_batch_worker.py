"""Worker for tests/test_gpu_multi_batch.py::test_every_plan_same_statuses: one blsgpu_multi_verify_batch call per sig_group over a
fixed mixed batch, in a fresh process (BLSGPU_MULTI_STRIP is read once, at library init).  Prints one JSON line:
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
    from multi_batch_cases import mixed_sets
    res = {}
    for sg in (1, 2):
        sets = mixed_sets(api, sg, api.BASIC, 70 + sg, sizes=(63, 64, 65, 130))
        res[sg] = api.multi_verify_batch(sg, api.BASIC, sets)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
