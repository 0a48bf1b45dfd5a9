"""Worker for tests/test_gpu_keyset.py::test_every_plan_same_statuses: the indexed multi and secure calls over a fixed batch, with and
without tables, in a fresh process (the BLSGPU_* knobs are read once, at library init).  Prints one JSON line."""
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
    import keyset_cases as kc
    res = {}
    for sg in (1, 2):
        t = kc.table(api, sg)
        rng = random.Random(300 + sg)
        multi = kc.multi_sets(api, sg, api.BASIC, t, rng)
        secure = kc.secure_sets(api, sg, api.BASIC, t, rng, sizes=[0, 1, 3, 65, 130])
        multi += kc.tampered(api, sg, multi) + [([kc.BAD, 1], multi[1][1], b'x'), ([2, kc.N], multi[1][1], b'y')]
        secure += [(secure[3][0], secure[3][1], b'other'), ([3, kc.BAD], secure[1][1], b'x')]
        for tables in (False, True):
            with api.KeySet.create(sg, t['blobs'], t['fmt'], tables=tables) as ks:
                res['%d/%d' % (sg, tables)] = dict(has_tables=ks.info()['has_tables'], multi=api.multi_verify_indexed_batch(ks, api.BASIC, multi),
                                                   secure=api.verify_secure_indexed_batch(ks, api.BASIC, secure),
                                                   sums=[s.hex() for s in api.serialize(3 - sg, api.sum_indexed_batch(ks, [m[0] for m in multi[:9]]))])
    print(json.dumps(res))


if __name__ == '__main__':
    main()
