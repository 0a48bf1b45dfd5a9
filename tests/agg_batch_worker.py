"""Worker for tests/test_gpu_agg_batch.py::test_every_plan_same_output: one blsgpu_aggregate_verify_batch call per (sig_group,
scheme) of RUNS over the case list plus one set above the default BLSGPU_AGG_BATCH_MAX, in a fresh process (the knob is read once,
at library init).  Prints one JSON line: {"<sig_group>-<scheme>": [[status, aux0, aux1], ...]}."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

BIG = 32800                                  # above the default BLSGPU_AGG_BATCH_MAX (32,768)
RUNS = [(1, 0), (2, 0), (1, 1), (2, 2)]      # Basic for both impls; MessageAugmentation and ProofOfPossession once each (no duplicate rule)


def plan_sets(api, sg, scheme):
    import agg_batch_cases as abc
    sets = abc.raw_sets(sg, abc.cases(sg, scheme))
    msgs = [b'plan %d' % i for i in range(BIG)]
    pks, sigs = api.sign_batch(sg, scheme, [1000 + 7 * i for i in range(BIG)], msgs)
    agg = api.point_sum(sg, sigs)
    # the large set in the middle of the list, valid; and once more at the end with its last message changed
    return sets[:5] + [(pks, msgs, agg)] + sets[5:] + [(pks, msgs[:-1] + [b'plan changed'], agg)]


def main():
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    api.init()
    res = {}
    for sg, scheme in RUNS:
        res['%d-%d' % (sg, scheme)] = [[st, a0, a1] for st, (a0, a1) in api.aggregate_verify_batch(sg, scheme, plan_sets(api, sg, scheme))]
    print(json.dumps(res))


if __name__ == '__main__':
    main()
