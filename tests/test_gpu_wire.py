"""blsgpu_verify_batch from wire bytes (BLSGPU_FMT_COMPRESSED / BLSGPU_FMT_LEGACY) on every kernel path and failure class.

A wire call decodes on the device (k_decompress, key first, then signature), skips the engine's small-batch forms and sends every
size through k_prepare + the two-pair pairing; an item that failed to decode leaves its pair slots unwritten and every later stage
must skip it on its status alone.  The cases and the status the reference gives each of them come from tests/wire_cases.py (the
oracle; tests/test_wire_cases.py checks the case list on the CPU); every comparison here is exact equality of status vectors.
Runs that need their own process (knobs are read once; one context; several logical devices) go through tests/wire_worker.py."""
import json
import os
import pickle
import subprocess
import sys

import pytest
import util
import wire_cases as w
from oracle.py import blsful_ref as ref

pytestmark = pytest.mark.gpu

COMPRESSED, LEGACY = w.FMT_COMPRESSED, w.FMT_LEGACY
FMT_IDS = {COMPRESSED: 'modern', LEGACY: 'legacy'}
SG_FMT = [(sg, fmt) for sg in (1, 2) for fmt in (COMPRESSED, LEGACY)]
SG_FMT_IDS = ['g%d-%s' % (sg, FMT_IDS[fmt]) for sg, fmt in SG_FMT]


def seeds_for(n, fmt):
    """below 64 items a batch is a prefix of the rotated kind list: one and two items take every rotation (every kind alone and
    as a neighbour), the sizes around a wave three of them"""
    return range(len(w.kinds(fmt))) if n <= 2 else (0, 11, 22) if n < 64 else (0,)


def diff(got, want, names):
    return [(i, names[i], got[i], want[i]) for i in range(len(want)) if i >= len(got) or got[i] != want[i]][:12]


def check_sizes(api, sg, scheme, fmt, sizes):
    for n in sizes:
        for seed in seeds_for(n, fmt):
            pks, sigs, msgs, want, names = w.build_batch(sg, scheme, fmt, n, seed)
            got = api.verify_batch(sg, scheme, pks, sigs, msgs, fmt=fmt)
            assert got == want, (n, seed, diff(got, want, names))


@pytest.mark.parametrize('sg,fmt', SG_FMT, ids=SG_FMT_IDS)
def test_every_size_class_pop(api, sg, fmt):
    """default knobs, scheme POP, every size the host branches on (wave and workgroup boundaries, BLSGPU_WIDE_MAX 512, 1,024,
    BLSGPU_COOP_MAX 4,096 and the lane-split kernels above it): the oracle's status vector, with undecodable items at item 0,
    item n - 1 and on both sides of the 32-, 64- and last 128-item boundaries"""
    check_sizes(api, sg, ref.POP, fmt, w.SIZES[sg])


@pytest.mark.parametrize('sg,fmt', SG_FMT, ids=SG_FMT_IDS)
@pytest.mark.parametrize('scheme', [ref.BASIC, ref.AUG], ids=['basic', 'aug'])
def test_size_classes_basic_and_aug(api, scheme, sg, fmt):
    """Basic and Aug (the augmentation prefix is built from the decoded key) at one size per plan"""
    check_sizes(api, sg, scheme, fmt, w.SIZES_THIN)


def test_beyond_one_chunk(api):
    """more items than one pass of the two-kernel Miller loop takes (70,001, the size of
    tests/test_gpu_fullsize.py::test_verify_batch_beyond_one_chunk): undecodable items in both chunks and on both sides of
    the chunk boundary"""
    sg, fmt, n = 1, COMPRESSED, 70001
    batch = w.build_batch(sg, ref.POP, fmt, n, 1)
    for pos, kind in ((65534, 'valid'), (65535, 'pk_offcurve'), (65536, 'sig_x_ge_p'), (65537, 'valid')):
        w.place(batch, sg, ref.POP, fmt, pos, kind, pos % w.POOL)
    pks, sigs, msgs, want, names = batch
    got = api.verify_batch(sg, ref.POP, pks, sigs, msgs, fmt=fmt)
    assert got == want, diff(got, want, names)


# ------------------------------------------------------------------ child processes
def run_worker(tmp_path, name, env, calls, devices=0, timeout=300):
    """one attempt: a worker that dies by a signal or outlives its limit fails the test, and nothing further is started"""
    path = str(tmp_path / (name + '.pickle'))
    with open(path, 'wb') as f:
        pickle.dump({'devices': devices, 'calls': calls}, f)
    keep = {k: v for k, v in os.environ.items() if not k.startswith('BLSGPU_') or k == 'BLSGPU_LIB'}
    r = subprocess.run([sys.executable, os.path.join(util.ROOT, 'tests', 'wire_worker.py'), path], env=dict(keep, **env),
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (name, env, r.returncode, r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def wire_call(sg, scheme, fmt, batch):
    return {'op': 'wire', 'sg': sg, 'scheme': scheme, 'fmt': fmt, 'pks': batch[0], 'sigs': batch[1], 'msgs': batch[2]}


@pytest.mark.parametrize('sg,fmt', SG_FMT, ids=SG_FMT_IDS)
def test_stale_pairs(tmp_path, sg, fmt):
    """one process, one context (BLSGPU_CONTEXTS=1), n in 40 (wave-cooperative), 600, 5,000 (lane-split): a RAW_PROJ call of n valid
    device-signed items, then a wire call of n valid items with the very messages of the next two (so its affine pairs stay where
    those calls have their pair slots), then the batch in which every item fails to decode -- no 0 anywhere -- and the one with a
    single survivor -- exactly one.  A stage that ran an undecodable item on what its slots held would report an earlier item's
    verdict."""
    calls, wants = [], []
    for n in (40, 600, 5000):
        calls.append({'op': 'raw_valid', 'sg': sg, 'scheme': ref.POP, 'n': n})
        wants.append(([0] * n, None))
        for layout in ('all_valid', 'all_fail', 'all_but_one'):
            b = w.build_batch(sg, ref.POP, fmt, n, n % 7, layout)
            calls.append(wire_call(sg, ref.POP, fmt, b))
            wants.append((b[3], b[4]))
            assert b[3].count(0) == {'all_valid': n, 'all_fail': 0, 'all_but_one': 1}[layout]
    got = run_worker(tmp_path, 'stale', {'BLSGPU_CONTEXTS': '1'}, calls)
    for k, (g, (want, names)) in enumerate(zip(got, wants)):
        assert g == want, (k, diff(g, want, names or [''] * len(want)))


def test_wire_equals_decode_then_raw(api):
    """on top of the oracle comparison: deserialize keys and signatures (statuses sk, ss), verify the decoded points as RAW_PROJ
    with a valid pair in place of what did not decode; the wire call's status is sk[i] or ss[i] or raw[i], item by item"""
    for sg, fmt in SG_FMT:
        for n in (129, 4097):
            pks, sigs, msgs, want, names = w.build_batch(sg, ref.POP, fmt, n, 2)
            legacy = fmt == LEGACY
            pk_raw, sk = api.deserialize(3 - sg, pks, legacy)
            sig_raw, ss = api.deserialize(sg, sigs, legacy)
            good = names.index('valid')
            assert sk[good] == ss[good] == 0
            for i in range(n):
                if sk[i] or ss[i]:
                    pk_raw[i], sig_raw[i] = pk_raw[good], sig_raw[good]
            raw = api.verify_batch(sg, ref.POP, pk_raw, sig_raw, msgs)
            wire = api.verify_batch(sg, ref.POP, pks, sigs, msgs, fmt=fmt)
            assert wire == [sk[i] or ss[i] or raw[i] for i in range(n)], (sg, fmt, n)
            assert wire == want, (sg, fmt, n, diff(wire, want, names))


PLANS = [
    ('lane_split', {'BLSGPU_COOP_MAX': '0'}, (40, 600)),                      # lane-split Miller / final exponentiation at every size
    ('no_wide', {'BLSGPU_WIDE_MAX': '0'}, (40, 600, 4200)),
    ('prepare_one_lane', {'BLSGPU_AB_KNOBS': '1', 'BLSGPU_PREPARE_LANES': '1'}, (40, 600, 4200)),
    ('finalexp_seg', {'BLSGPU_AB_KNOBS': '1', 'BLSGPU_FINALEXP_SEG': '1'}, (40, 600, 4200)),
    ('first_generation', {'BLSGPU_AB_KNOBS': '1', 'BLSGPU_MILLER_V1': '1', 'BLSGPU_FINALEXP_V1': '1'}, (40, 600, 4200)),
]


@pytest.mark.parametrize('name,env,sizes', PLANS, ids=[p[0] for p in PLANS])
def test_every_plan(tmp_path, api, name, env, sizes):
    """every plan the switches select gives the default plan's status vectors and the oracle's, both orientations and formats"""
    batches = [(sg, fmt, w.build_batch(sg, ref.POP, fmt, n, 3)) for sg, fmt in SG_FMT for n in sizes]
    got = run_worker(tmp_path, name, env, [wire_call(sg, ref.POP, fmt, b) for sg, fmt, b in batches])
    for g, (sg, fmt, b) in zip(got, batches):
        assert g == b[3], (name, sg, fmt, len(b[3]), diff(g, b[3], b[4]))
        assert g == api.verify_batch(sg, ref.POP, b[0], b[1], b[2], fmt=fmt), (name, sg, fmt, len(b[3]))


@pytest.mark.parametrize('D', [2, 3])
def test_sharded(tmp_path, D):
    """the in-library multi-device split (BLSGPU_FAKE_DEVICES logical devices on one GPU, BLSGPU_SHARD_MIN below n): shard d takes
    items [n d / D, n (d + 1) / D) at key strides of 48 / 96 and signature strides of 96 / 48 bytes and writes statuses at its
    offset; an undecodable item is the last of every shard and the first of the next"""
    batches = []
    for sg, fmt in SG_FMT:
        for n in (1000, 1001):
            b = w.build_batch(sg, ref.POP, fmt, n, D)
            for d in range(1, D):
                lo = n * d // D
                w.place(b, sg, ref.POP, fmt, lo - 2, 'valid', lo % w.POOL)
                w.place(b, sg, ref.POP, fmt, lo - 1, 'sig_offcurve', lo % w.POOL)
                w.place(b, sg, ref.POP, fmt, lo, 'pk_hdr1', (lo + 1) % w.POOL)
                w.place(b, sg, ref.POP, fmt, lo + 1, 'valid', (lo + 1) % w.POOL)
            batches.append((sg, fmt, b))
    got = run_worker(tmp_path, 'shard%d' % D, {'BLSGPU_FAKE_DEVICES': str(D), 'BLSGPU_SHARD_MIN': '64'},
                     [wire_call(sg, ref.POP, fmt, b) for sg, fmt, b in batches], devices=D)
    for g, (sg, fmt, b) in zip(got, batches):
        assert g == b[3], (D, sg, fmt, len(b[3]), diff(g, b[3], b[4]))


def test_device_resident(tmp_path):
    """wire bytes, message blob, offsets and the status vector on the device, n = 700"""
    batches = [(sg, fmt, w.build_batch(sg, ref.POP, fmt, 700, 4)) for sg, fmt in SG_FMT]
    got = run_worker(tmp_path, 'device', {}, [dict(wire_call(sg, ref.POP, fmt, b), op='wire_device') for sg, fmt, b in batches])
    for g, (sg, fmt, b) in zip(got, batches):
        assert g == b[3], (sg, fmt, diff(g, b[3], b[4]))


def test_aug_prefix_from_legacy_bytes(api):
    """Bls12381G2Impl, Aug, LEGACY input, keys whose y-sign bit is set (legacy byte 0 differs from the modern one): the
    augmentation prefix is what the reference's to_bytes() yields -- the modern bytes -- so the pool's items verify, and a
    signature over H(legacy key bytes || m) does not (a library that prefixed the caller's bytes would accept it)"""
    C, sg, scheme = ref.G2Impl, 2, ref.AUG
    cs = w.cases(sg, scheme, LEGACY)
    pks, sigs, msgs, want = [], [], [], []
    for j, (pkb, _, msg, _, _, sk) in enumerate(w.pool(sg, scheme)):
        if not pkb[0] & 0x20:
            continue
        leg = ref.modern_to_legacy(pkb)
        assert leg[0] != pkb[0]
        item = cs['valid', j]
        assert item[0] == leg and item[3] == 0
        forged = C.sig_to_bytes(C.sig_curve.mul(C.hash_to_point(leg + msg, C.DST[scheme]), sk))
        for sigb in (item[1], ref.modern_to_legacy(forged)):
            pks.append(leg)
            sigs.append(sigb)
            msgs.append(msg)
            want.append(w.expected_status(sg, scheme, LEGACY, leg, sigb, msg))
    assert len(want) >= 2 and want == [0, 1] * (len(want) // 2)
    assert api.verify_batch(sg, scheme, pks, sigs, msgs, fmt=LEGACY) == want


@pytest.mark.parametrize('sg,fmt', SG_FMT, ids=SG_FMT_IDS)
def test_deserialize_columns(api, sg, fmt):
    """blsgpu_deserialize (and, for modern signatures, blsgpu_signatures_from_tagged) on the 4,097 keys and signatures of a batch:
    the oracle's decode statuses, and what decoded serialises back to the oracle's modern bytes"""
    C = w.IMPLS[sg]
    pks, sigs, _, _, _ = w.build_batch(sg, ref.POP, fmt, 4097, 6)
    for group, blobs, comp in ((3 - sg, pks, C.pk_to_bytes), (sg, sigs, C.sig_to_bytes)):
        dec = [w.decode(48 * group, b, fmt) for b in blobs]
        pts, st = api.deserialize(group, blobs, fmt == LEGACY)
        assert st == [d[0] for d in dec], diff(st, [d[0] for d in dec], [b.hex()[:8] for b in blobs])
        ok = [i for i, d in enumerate(dec) if d[0] == 0]
        assert len(ok) > 1000 and len(ok) < len(dec) - 500
        assert api.serialize(group, [pts[i] for i in ok]) == [comp(dec[i][1]) for i in ok]
    if fmt == COMPRESSED:
        dec = [w.decode(C.SIG_BYTES, b, fmt) for b in sigs]
        tags, pts, st = api.signatures_from_tagged(sg, [bytes([i % 3]) + b for i, b in enumerate(sigs)])
        ok = [i for i, d in enumerate(dec) if d[0] == 0]
        assert st == [d[0] for d in dec] and [tags[i] for i in ok] == [i % 3 for i in ok]
        assert api.serialize(sg, [pts[i] for i in ok]) == [C.sig_to_bytes(dec[i][1]) for i in ok]
