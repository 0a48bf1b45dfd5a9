"""Worker for tests/test_gpu_msm.py: runs a list of MSM / verify_secure / aggregate_secure cases in a fresh process (the
BLSGPU_* knobs are read once, at library init) and prints one JSON line of results.
argv: spec.json (written by the test; see tests/test_gpu_msm.py for the case format)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def device_points(api, group, sks):
    """{sk: RAW_PROJ point sk * g of `group`}, made on the device (public keys of the other orientation)."""
    sks = sorted(set(sks))
    if not sks:
        return {}
    pks, _ = api.sign_batch(3 - group, api.BASIC, sks, [b''] * len(sks))
    return dict(zip(sks, pks))


def run_msm(api, util, spec):
    out = []
    for group in (1, 2):
        cases = [cs for cs in spec['msm'] if cs['group'] == group]
        pts = device_points(api, group, [e for cs in cases for e in cs['pts'] if isinstance(e, int)])
        ident = util.g1_raw(None) if group == 1 else util.g2_raw(None)
        for cs in cases:
            row = [ident if e is None else pts[e] if isinstance(e, int) else bytes.fromhex(e) for e in cs['pts']]
            ts = [int(t, 16) for t in cs['ts']]
            got = api.serialize(group, [api.point_sum(group, row, ts, fmt=cs.get('fmt', api.FMT_RAW_PROJ))])[0]
            out.append([cs['name'], got.hex()])
    return out


def run_secure(api, spec):
    out = []
    for cs in spec['secure']:
        sg, msg = cs['sg'], cs['msg'].encode()
        keys = device_points(api, 3 - sg, cs['sks'])
        pks = [keys[s] for s in cs['sks']]
        _, sigs = api.sign_batch(sg, api.BASIC, cs['sig_sks'], [msg] * len(cs['sig_sks']))
        out.append([cs['name'], [api.verify_secure(sg, api.BASIC, pks, sig, msg) for sig in sigs]])
    return out


def run_aggregate(api, spec):
    out = []
    for cs in spec['aggregate']:
        sg, msg = cs['sg'], cs['msg'].encode()
        keys = device_points(api, 3 - sg, cs['sks'])
        pks = [keys[s] for s in cs['sks']]
        _, sigs = api.sign_batch(sg, api.BASIC, cs['sig_sks'], [msg] * len(cs['sig_sks']))
        st, agg = api.aggregate_secure(sg, pks, sigs)
        out.append([cs['name'], st, api.serialize(sg, [agg])[0].hex()])
    return out


def main():
    spec = json.load(open(sys.argv[1]))
    import util
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    api.init()
    res = {'msm': run_msm(api, util, spec), 'secure': run_secure(api, spec), 'aggregate': run_aggregate(api, spec)}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
