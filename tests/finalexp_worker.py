"""Worker for tests/test_gpu_finalexp.py: runs the batch final exponentiation forms (blsgpu_debug_finalexp_batch) and the product
forms (blsgpu_fp12_product_is_one) on the cases of a spec in a fresh process (the BLSGPU_* knobs are read once, at library init)
and prints one JSON line of results.
argv: spec.json records.bin -- the spec names records by index into records.bin (576 bytes each)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    spec = json.load(open(sys.argv[1]))
    blob = open(sys.argv[2], 'rb').read()
    rec = [blob[576 * i:576 * (i + 1)] for i in range(len(blob) // 576)]
    import __graft_entry__ as ge
    api = ge.import_pkg().api
    api.init()
    res = {'batch': [], 'product': []}
    for cs in spec['batch']:
        st = api.debug_finalexp_batch([rec[i] for i in cs['records']], cs['form'], cs['chunk'], cs['status'])
        res['batch'].append([cs['name'], st])
    for cs in spec['product']:
        res['product'].append([cs['name'], api.fp12_product_is_one([rec[i] for i in cs['records']])])
    print(json.dumps(res))


if __name__ == '__main__':
    main()
