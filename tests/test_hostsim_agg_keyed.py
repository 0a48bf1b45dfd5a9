"""The host side of the keyed line kernel of the batched aggregate verify over a registered key set (k_linesp_keyed; csrc/pairing.cuh
miller_line3_row, csrc/keyset.cuh keyset_lines_entry, csrc/agg_batch.cuh agg_batch_plan / agg_flat_pair / agg_flat_key /
agg_round_size) with the bound tracker on, on the host emulation of the lane-split tower.  Every item is one pair whose G2 member is
given as 68 normalised rows -- a key's built rows, or the rows of -[c] g2 -- and its line values are the keyed kernel's entry
function; they go through the one-pair Miller accumulation and, multiplied over a set, the final exponentiation.  Verdicts are
compared with the oracle's AggregateSignature::verify (never raw Miller values: normalised rows differ from walked lines by factors
in Fp2).  The flat-index map is checked with integers only.  A violated bound aborts the process, so a test that returns has seen
the tracker silent.  The same driver runs once more as a stand-alone program under the address and undefined-behaviour sanitizers
(a host build, nothing preloaded)."""
import ctypes
import os
import random
import subprocess
import tempfile

import pytest

import util
from util import c, ref

SRC = os.path.join(util.ROOT, 'tests', 'hostsim_agg_keyed', 'agg_keyed_hostsim.cpp')
SIG_ITEM = 0xfffffffe


@pytest.fixture(scope='module')
def lib():
    so = os.path.join(tempfile.mkdtemp(prefix='agg_keyed_hostsim_'), 'libagg_keyed_hostsim.so')
    subprocess.check_call(['g++', '-O2', '-DBLS_TRACK_BOUNDS', '-shared', '-fPIC', '-o', so, SRC])
    lb = ctypes.CDLL(so)
    lb.hs_product_verdict.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p]
    lb.hs_flat_map.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                               ctypes.c_void_p]
    lb.hs_flat_map.restype = ctypes.c_long
    lb.hs_round_size.argtypes = [ctypes.c_size_t, ctypes.c_size_t]
    lb.hs_round_size.restype = ctypes.c_size_t
    return lb


def uncleared_hash(msg, dst):
    """the message point the Bls12381G1Impl kernels pair with: the sum of the two mapped points, before the cofactor is cleared"""
    u0, u1 = c.hash_to_field(msg, dst, 2, 1)
    q = c.E1.add(c.map_to_curve_g1(u0), c.map_to_curve_g1(u1))
    assert c.E1.mul(q, c.H_EFF_G1) == c.hash_to_g1(msg, dst)
    return q


def negc():
    return c.E2.neg(c.E2.mul(c.G2_GEN, pow(c.H_EFF_G1, -1, c.R)))


C = ref.G1Impl
DST = C.DST[ref.POP]


@pytest.fixture(scope='module')
def signers():
    rng = random.Random(17)
    sks = [rng.randrange(1, c.R) for _ in range(4)]
    pks = [C.pk_curve.mul(C.pk_gen, sk) for sk in sks]
    msgs = [b'keyed aggregate %d' % i for i in range(4)]
    sigs = [C.sig_curve.mul(c.hash_to_g1(m, DST), sk) for sk, m in zip(sks, msgs)]
    return sks, pks, msgs, sigs


def oracle(pks, msgs, sig):
    try:
        ref.aggregate_verify(C, ref.POP, list(zip(pks, msgs)), sig)
        return 0
    except ref.BlsError as e:
        assert e.kind == 'InvalidSignature', e
        return 1


def from_rows(lib, pks, msgs, sig, built_negc=False):
    recs = b''.join(util.g2_aff_raw(p) for p in pks)
    pts = b''.join(util.g1_aff_raw(uncleared_hash(m, DST)) for m in msgs) + util.g1_aff_raw(sig)
    return lib.hs_product_verdict(recs, pts, len(pks), util.g2_aff_raw(negc()) if built_negc else None)


def total(sigs):
    s = None
    for g in sigs:
        s = g if s is None else C.sig_curve.add(s, g)
    return s


def test_one_pair_verdicts_from_rows(lib, signers):
    """one (key, message, signature) tuple = one pair item times the signature item: the oracle's verdict on the valid tuple and on the
    tuple with the key, the message or the signature of another signer; the rows of -[c] g2 built through the key-set path and
    the generated table give the same"""
    sks, pks, msgs, sigs = signers
    for i in range(3):
        j = i + 1
        for pk, m, s in ((pks[i], msgs[i], sigs[i]), (pks[j], msgs[i], sigs[i]), (pks[i], msgs[j], sigs[i]), (pks[i], msgs[i], sigs[j])):
            want = oracle([pk], [m], s)
            assert want == (0 if (pk, m, s) == (pks[i], msgs[i], sigs[i]) else 1)
            assert from_rows(lib, [pk], [m], s) == want, i
            assert from_rows(lib, [pk], [m], s, built_negc=True) == want, i


@pytest.mark.parametrize('n', [1, 2, 3])
def test_products_from_rows(lib, signers, n):
    """n pairs times the signature item: a valid set, the set with one message changed and the set with one key swapped"""
    sks, pks, msgs, sigs = signers
    agg = total(sigs[:n])
    cases = [(pks[:n], msgs[:n], 0),
             (pks[:n], msgs[:n - 1] + [b'another message'], 1),
             (pks[:n - 1] + [pks[3]], msgs[:n], 1)]
    for ks, ms, want in cases:
        assert oracle(ks, ms, agg) == want
        assert from_rows(lib, ks, ms, agg) == want


def test_refused_rows_are_reported(lib, signers):
    """the identity record has no rows: the driver says so and evaluates nothing (the kernel skips such an item by its flag)"""
    sks, pks, msgs, sigs = signers
    pts = util.g1_aff_raw(uncleared_hash(msgs[0], DST)) + util.g1_aff_raw(sigs[0])
    assert lib.hs_product_verdict(bytes(192), pts, 1, None) == -1


def flat_map(lib, sizes, max_small, per_round):
    T = sum(sizes)
    cidx = (ctypes.c_uint32 * max(T, 1))(*[7000 + 3 * p for p in range(T)])           # position p names entry 7000 + 3 p
    cap = T + len(sizes) + 1
    key, src, first = (ctypes.c_uint32 * cap)(), (ctypes.c_uint32 * cap)(), (ctypes.c_uint64 * cap)()
    M = lib.hs_flat_map((ctypes.c_uint64 * len(sizes))(*sizes), len(sizes), max_small, per_round, cidx, key, src, first)
    assert M >= 0
    return M, list(key)[:M], list(src)[:M], list(first)[:M]


LARGE = 9


@pytest.mark.parametrize('per_round', [32, 4, 1, 5])
def test_flat_index_map(lib, per_round):
    """sets of 0, 3, LARGE, 1, 0, 2 pairs with the large-set threshold between 3 and LARGE: the flat list holds the batched sets'
    pairs, set after set, then one signature item per batched set; every pair item resolves to the entry its OWN caller position
    names, whatever round takes it -- rounds of 4, 1 and 5 items start at a non-zero `first` inside the pair items, between them
    and the signature items, and inside those"""
    sizes = [0, 3, LARGE, 1, 0, 2]
    offs = [sum(sizes[:s]) for s in range(len(sizes) + 1)]
    batched = [s for s, t in enumerate(sizes) if t < 5]
    want_src = [p for s in batched for p in range(offs[s], offs[s + 1])]
    T_b = len(want_src)
    M, key, src, first = flat_map(lib, sizes, 5, per_round)
    assert M == T_b + len(batched) == 11
    assert src[:T_b] == want_src == [0, 1, 2, 12, 13, 14]                    # not the flat index: the large set's 9 positions lie between
    assert key[:T_b] == [7000 + 3 * p for p in want_src]
    assert key[T_b:] == [SIG_ITEM] * len(batched) and src[T_b:] == batched
    assert first == [i // per_round * per_round for i in range(M)]


def test_flat_index_map_without_batched_or_large_sets(lib):
    assert flat_map(lib, [LARGE, LARGE + 1], 5, 32)[0] == 0                  # only large sets: no flat list
    M, key, src, _ = flat_map(lib, [0, 0], 5, 32)                            # only empty sets: two signature items
    assert M == 2 and key == [SIG_ITEM] * 2 and src == [0, 1]
    M, key, src, _ = flat_map(lib, [2, 3], 5, 32)
    assert M == 7 and src == [0, 1, 2, 3, 4, 0, 1]


def test_round_size(lib):
    """rounds of equal size, a multiple of 32, at most one machine round of lane pairs, that cover the list; 1,040 sets of 63
    pairs (66,560 items) take two rounds, the second from a non-zero `first`"""
    for M in (0, 1, 31, 32, 33, 65535, 65536, 65537, 66560, 131072, 131073, 300000):
        r = lib.hs_round_size(M, 65536)
        if M == 0:
            assert r == 0
            continue
        assert r % 32 == 0 and 0 < r <= 65536
        rounds = -(-M // r)
        assert rounds == -(-M // 65536) and rounds * r >= M
    assert lib.hs_round_size(66560, 65536) == 33280


def test_standalone_under_sanitizers():
    exe = os.path.join(tempfile.mkdtemp(prefix='agg_keyed_hostsim_san_'), 'agg_keyed_hostsim')
    subprocess.check_call(['g++', '-O1', '-g', '-DBLS_TRACK_BOUNDS', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-DAGG_KEYED_HOSTSIM_MAIN', '-o', exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr[-2000:]
    assert p.stdout.strip().endswith(' 0 bad')
