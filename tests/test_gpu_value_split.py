"""Pairing values on the lane-split kernels (BLSGPU_VALUE_SPLIT_MIN): blsgpu_pairing_batch, blsgpu_timecrypt_open_batch,
blsgpu_pairing_sigset_batch and blsgpu_timecrypt_open_indexed_batch under the plan that runs k_linesp / k_millerfp3 or k_millerf_rows1
and then k_finalexp2s_value, and blsgpu_debug_finalexp_value on crafted Fp12 records.  Bytes, messages and statuses are exact, and
every expectation comes from tests/timecrypt_cases.py, tests/sigset_cases.py and tests/finalexp_cases.py -- the oracle --, never from
another GPU run; the plan of every call is read from its launches (blsgpu_profile_get).  The knobs are parsed once per process, so each
plan runs in a fresh child (tests/value_split_worker.py), one attempt, with a limit of its own."""
import functools
import os
import pickle
import random
import subprocess
import sys

import pytest

import finalexp_cases as fc
import sigset_cases as sc
import timecrypt_cases as tc
import timecrypt_ref as tr
import util
from util import c

pytestmark = pytest.mark.gpu

VALUE, ROWS1, LINESP, MILLERFP = 'k_finalexp2s_value', 'k_millerf_rows1', 'k_linesp', 'k_millerfp'
ONE_WAVE = ('k_pairing_value', 'k_pairing_value_rows')
SPLIT = {'BLSGPU_VALUE_SPLIT_MIN': '1'}
SPLIT_CHUNK64 = dict(SPLIT, BLSGPU_AB_KNOBS='1', BLSGPU_MILLER_CHUNK='64')
VALUE_SPLIT_MIN_DEFAULT = 8192     # csrc/blsgpu.hip VALUE_SPLIT_MIN_DEFAULT: the measured default


def run_worker(tmp_path, name, calls, env, records=None, timeout=240):
    """one attempt: a worker that dies by a signal or outlives its limit fails the test, and nothing further is started"""
    spec, out = str(tmp_path / (name + '.spec.pickle')), str(tmp_path / (name + '.out.pickle'))
    with open(spec, 'wb') as f:
        pickle.dump({'calls': calls, 'records': records}, f)
    keep = {k: v for k, v in os.environ.items() if not k.startswith('BLSGPU_') or k == 'BLSGPU_LIB'}
    r = subprocess.run([sys.executable, os.path.join(util.ROOT, 'tests', 'value_split_worker.py'), spec, out], env=dict(keep, **env), capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, (name, r.returncode, r.stderr[-3000:])
    with open(out, 'rb') as f:
        return pickle.load(f)


def split(blob, n):
    assert len(blob) == tr.GT_BYTES * n
    return [blob[tr.GT_BYTES * i:tr.GT_BYTES * (i + 1)] for i in range(n)]


def diff(got, want):
    return [(i, got[i][:8].hex(), want[i][:8].hex()) for i in range(len(want)) if got[i] != want[i]][:8]


def walked(k):
    """the lane-split plan with every pair walked, and nothing of the one-wave plan"""
    return VALUE in k and LINESP in k and MILLERFP in k and k[LINESP] == k[MILLERFP] == k[VALUE] and ROWS1 not in k and not any(x in k for x in ONE_WAVE)


def tabled(k):
    """the lane-split plan with every line read from the set's rows"""
    return VALUE in k and ROWS1 in k and k[ROWS1] == k[VALUE] and LINESP not in k and MILLERFP not in k and not any(x in k for x in ONE_WAVE)


def mixed_batch(fmt, n, seed):
    """n items: the special ones (identities on either side, P and -P, on the wire formats the pairs that do not decode) shuffled among
    running pairs, so that they share a wave; n = 1: one running pair; n = 2: a running pair and an identity"""
    names, s1, s2, sw, sst = tc.special_items(fmt)
    k = 0 if n == 1 else 1 if n == 2 else len(names)
    first = names.index('identity G1') if n == 2 else 0
    g1s, g2s, want, st = tc.items(fmt, n - k, seed=seed)
    g1s, g2s, want, st = g1s + s1[first:first + k], g2s + s2[first:first + k], want + sw[first:first + k], st + sst[first:first + k]
    order = list(range(n))
    random.Random(seed).shuffle(order)
    pick = lambda xs: [xs[i] for i in order]  # noqa: E731
    return pick(g1s), pick(g2s), pick(want), pick(st)


# ------------------------------------------------------------------ pairing values
@pytest.mark.parametrize('fmt', tc.FMTS, ids=[tc.FMT_IDS[f] for f in tc.FMTS])
def test_pairing_values_at_small_sizes(tmp_path, fmt):
    """n = 1, 2, 31, 32, 33 (a workgroup is 64 lanes: 32 items) and 65 under BLSGPU_VALUE_SPLIT_MIN=1: bytes and statuses exact, and
    the launches are the lane-split plan's"""
    batches = [mixed_batch(fmt, n, seed=n) for n in (1, 2, 31, 32, 33, 65)]
    assert any(w == tr.GT_ONE for w in batches[2][2]) and (fmt in (tc.RAW_PROJ, tc.RAW_AFFINE) or any(w == tc.ZERO_GT for w in batches[2][2]))
    got = run_worker(tmp_path, 'small', [{'op': 'pairing', 'g1s': b[0], 'g2s': b[1], 'fmt': fmt} for b in batches], SPLIT)
    for (k, blob, gst), b in zip(got, batches):
        rec = split(blob, len(b[2]))
        assert gst == b[3], (fmt, len(b[2]), gst)
        assert rec == b[2], (fmt, len(b[2]), diff(rec, b[2]))
        assert walked(k) and k[VALUE] == 1, (fmt, len(b[2]), k)


def test_chunk_boundaries(tmp_path):
    """BLSGPU_MILLER_CHUNK=64 and 129 items: three chunks, two with first > 0 -- host arguments, then every argument and result in
    device memory"""
    b = mixed_batch(tc.COMPRESSED, 129, seed=9)
    call = {'g1s': b[0], 'g2s': b[1], 'fmt': tc.COMPRESSED}
    got = run_worker(tmp_path, 'chunks', [dict(call, op='pairing'), dict(call, op='pairing_device')], SPLIT_CHUNK64)
    for k, blob, gst in got:
        rec = split(blob, 129)
        assert gst == b[3] and rec == b[2], diff(rec, b[2])
        assert walked(k) and k[VALUE] == 3, k


def test_the_default_plan_is_unchanged_below_the_threshold(tmp_path):
    """no BLSGPU_ variable, 65 items: k_pairing_value and none of the lane-split kernels"""
    b = mixed_batch(tc.RAW_PROJ, 65, seed=3)
    (k, blob, gst), = run_worker(tmp_path, 'default', [{'op': 'pairing', 'g1s': b[0], 'g2s': b[1], 'fmt': tc.RAW_PROJ}], {})
    assert gst == b[3] and split(blob, 65) == b[2]
    assert k.get('k_pairing_value') == 1 and not any(x in k for x in (VALUE, ROWS1, LINESP, MILLERFP, 'k_pairing_value_rows')), k


def test_one_item_above_the_measured_default(tmp_path):
    """no BLSGPU_ variable, the default plus one items -- the dozen distinct pairs repeated, the expected bytes tiled: exact, and on
    the lane-split plan"""
    src = open(os.path.join(util.ROOT, 'agora-blsful_amd', 'csrc', 'blsgpu.hip')).read()
    assert '#define VALUE_SPLIT_MIN_DEFAULT %d\n' % VALUE_SPLIT_MIN_DEFAULT in src
    n = VALUE_SPLIT_MIN_DEFAULT + 1
    one = tc.items(tc.RAW_AFFINE, len(tc.SCALARS))
    rep = lambda xs: [xs[i % len(xs)] for i in range(n)]  # noqa: E731
    (k, blob, gst), = run_worker(tmp_path, 'at_default', [{'op': 'pairing', 'g1s': rep(one[0]), 'g2s': rep(one[1]), 'fmt': tc.RAW_AFFINE}], {})
    rec = split(blob, n)
    assert gst == [0] * n and rec == rep(one[2]), diff(rec, rep(one[2]))
    assert walked(k), k


# ------------------------------------------------------------------ crafted Fp12 inputs
@functools.lru_cache(maxsize=None)
def pool():
    """[(name, family, value, the oracle's Gt bytes)] of the families S, K, N and M; Z (the zero element) is left out: no public call
    can produce it and its bytes are not specified"""
    return [(name, fam, v, tr.gt_bytes(c.final_exponentiation(v))) for name, fam, v in fc.family_pool() if fam != 'Z']


def test_crafted_fp12_records(tmp_path):
    """blsgpu_debug_finalexp_value: the families shuffled together so that decliners (S: the easy part is 1, the compressed chain
    declines; the value must be Gt one) and compressed items share a wave; n = 1, 2, 63, 64, 65, 129 with the library's chunk and 64;
    preset flags come back as the constant records"""
    pl = pool()
    names = [p[0] for p in pl]
    assert {p[1] for p in pl} == {'S', 'K', 'N', 'M'} and all(p[3] == tr.GT_ONE for p in pl if p[1] == 'S') and any(p[3] != tr.GT_ONE for p in pl)
    records = [fc.record(p[2]) for p in pl]
    rng = random.Random(23)
    calls, want = [], []
    for n in (1, 2, 63, 64, 65, 129):
        if n == 1:
            order = [names.index('y^r*z_0')]
        elif n == 2:
            order = [names.index('fp6_0'), names.index('y_0')]
        else:
            order = []
            while len(order) < n:
                order += rng.sample(range(len(pl)), len(pl))
            order = order[:n]
        flags = [1 if n > 2 and i % 9 == 4 else 2 if n > 2 and i % 13 == 7 else 0 for i in range(n)]
        w = [tr.GT_ONE if f == 1 else tc.ZERO_GT if f == 2 else pl[o][3] for f, o in zip(flags, order)]
        for chunk in (0, 64):
            calls.append({'op': 'finalexp_value', 'records': order, 'chunk': chunk, 'flags': flags})
            want.append((n, chunk, w, [names[o] for o in order]))
    got = run_worker(tmp_path, 'crafted', calls, {}, records=records)
    bad = []
    for (k, blob), (n, chunk, w, labels) in zip(got, want):
        rec = split(blob, n)
        bad += [(n, chunk, i, labels[i], rec[i][:8].hex(), w[i][:8].hex()) for i in range(n) if rec[i] != w[i]]
        assert k[VALUE] == (1 if chunk == 0 else (n + 63) // 64), (n, chunk, k)
    assert not bad, bad[:20]


# ------------------------------------------------------------------ time-lock opening
@pytest.mark.parametrize('sg', [1, 2])
def test_timelock_opening(tmp_path, sg):
    """the whole case list of tests/timecrypt_cases.py (every status, the frame rules) as one call per format, on the lane-split plan"""
    rendered = [tc.render_groups(sg, tc.timelock_groups(sg), fmt) for fmt in tc.FMTS]
    got = run_worker(tmp_path, 'open%d' % sg, [{'op': 'timecrypt', 'sg': sg, 'groups': r[0], 'fmt': fmt} for r, fmt in zip(rendered, tc.FMTS)], SPLIT)
    for (k, msgs, sts), (_, want_msgs, want_sts), fmt in zip(got, rendered, tc.FMTS):
        bad = [(i, sts[i], want_sts[i]) for i in range(len(want_sts)) if sts[i] != want_sts[i] or msgs[i] != want_msgs[i]]
        assert len(sts) == len(want_sts) and not bad, (sg, fmt, bad[:8])
        assert tc.OK in sts and walked(k) and 'k_timecrypt_open' in k, (sg, fmt, k)


# ------------------------------------------------------------------ signature sets
def the_set(sg, entries, fmt, lines, **more):
    return dict({'sg': sg, 'sigs': [b for b, _ in entries], 'tags': [t for _, t in entries], 'fmt': fmt, 'lines': lines}, **more)


def test_signature_sets_open_by_index(tmp_path):
    """blsgpu_timecrypt_open_indexed_batch under the knob.  A Bls12381G2Impl set with rows takes k_millerf_rows1 (the two items that
    name no entry answer BLSGPU_E_ARG in their slots); the same set without rows, a Bls12381G1Impl set with the flag, and the full case
    list -- which names the identity entry and, on the wire, an undecodable one: entries without usable rows -- take the walked plan;
    entries appended after creation are read through their rows"""
    fmt = tc.RAW_AFFINE
    calls, want = [], []
    for sg, lines, plan in ((2, True, tabled), (2, False, walked), (1, True, walked)):
        entries, est, items, msgs, sts, _ = sc.render(sg, fmt, groups=sc.rows_groups(sg))
        calls.append({'op': 'sigset_open', 'items': items, 'fmt': fmt, 'set': the_set(sg, entries, fmt, lines)})
        want.append((plan, est, msgs, sts))
    for f in (tc.RAW_AFFINE, tc.COMPRESSED):
        entries, est, items, msgs, sts, _ = sc.render(2, f)
        calls.append({'op': 'sigset_open', 'items': items, 'fmt': f, 'set': the_set(2, entries, f, True)})
        want.append((walked, est, msgs, sts))
    entries, est, items, msgs, sts, _ = sc.render(2, fmt, groups=sc.rows_groups(2))
    grown = the_set(2, entries[:2], fmt, True, append=[([b for b, _ in entries[2:]], [t for _, t in entries[2:]], fmt)])
    calls.append({'op': 'sigset_open', 'items': items, 'fmt': fmt, 'set': grown})
    want.append((tabled, est[:2], msgs, sts))
    assert len(entries) > 3 and any(it[0] >= 2 for it in items)
    got = run_worker(tmp_path, 'sets', calls, SPLIT)
    for n, ((k, gest, gmsgs, gsts), (plan, est, msgs, sts)) in enumerate(zip(got, want)):
        assert gest == est and gsts == sts and gmsgs == msgs, (n, [(i, a, b) for i, (a, b) in enumerate(zip(gsts, sts)) if a != b][:8])
        assert plan(k), (n, k)
    assert sc.E_ARG in want[0][3] and tc.OK in want[0][3]
    assert any(s != tc.OK for s in want[3][1] + want[4][1])          # the full list holds an entry that did not decode or is the identity


@pytest.mark.parametrize('sg', [1, 2])
def test_signature_sets_pairing_values_by_index(tmp_path, sg):
    """blsgpu_pairing_sigset_batch under the knob with BLSGPU_MILLER_CHUNK=64: 70 plain pairs by index over 13 entries with rows (two
    chunks; Bls12381G2Impl reads the rows), then the special pairs too, with an identity entry named (every item walks) and one index
    outside the set (BLSGPU_E_ARG and 576 zero bytes in its slot)"""
    fmt = tc.RAW_PROJ
    g1s, g2s, want, st = tc.items(fmt, 13)
    names, a1, a2, w, s = tc.special_items(fmt)
    ents, pts = (g1s, g2s) if sg == 1 else (g2s, g1s)
    idx = [(7 * i) % 13 for i in range(70)]
    e_all, p_all = (g1s + a1, g2s + a2) if sg == 1 else (g2s + a2, g1s + a1)
    n_all = len(e_all)
    idx2 = list(range(n_all))[::-1] + [n_all]
    got = run_worker(tmp_path, 'values%d' % sg, [
        {'op': 'sigset_pairing', 'idx': idx, 'points': [pts[k] for k in idx], 'fmt': fmt, 'set': the_set(sg, [(b, 0) for b in ents], fmt, True)},
        {'op': 'sigset_pairing', 'idx': idx2, 'points': [p_all[k] for k in idx2[:-1]] + [p_all[0]], 'fmt': fmt, 'set': the_set(sg, [(b, 0) for b in e_all], fmt, True)}],
        SPLIT_CHUNK64)
    k, est, blob, gst = got[0]
    rec = split(blob, 70)
    assert est == [tc.OK] * 13 and gst == [tc.OK] * 70 and rec == [want[k] for k in idx], diff(rec, [want[k] for k in idx])
    assert (tabled(k) if sg == 2 else walked(k)) and k[VALUE] == 2, k
    k, est, blob, gst = got[1]
    w_all, s_all = want + w, st + s
    rec = split(blob, n_all + 1)
    assert gst == [s_all[k] for k in idx2[:-1]] + [sc.E_ARG]
    assert rec == [w_all[k] for k in idx2[:-1]] + [tc.ZERO_GT], diff(rec, [w_all[k] for k in idx2[:-1]] + [tc.ZERO_GT])
    assert walked(k), k
