"""CPU side of the wire-format verify_batch tests: the case list of tests/wire_cases.py keeps its promises (every kind and every
status in every batch, decode failures next to valid items where the kernels change plan, no kind dropped silently), the
oracle's expectations hold for the reference's own vectors, and the host-compiled copy of the device decompression gives the
oracle's decode status for every crafted key and signature encoding.  Runs without a GPU; tests/test_gpu_wire.py runs the same
cases on the device."""
import ctypes
import json
import os

import pytest
import util
import wire_cases as w
from oracle.py import blsful_ref as ref

FMTS = (w.FMT_COMPRESSED, w.FMT_LEGACY)
COMBOS = [(sg, scheme, fmt) for sg in (1, 2) for scheme in (ref.BASIC, ref.AUG, ref.POP) for fmt in FMTS]
IDS = ['g%d-%s-%s' % (sg, ('basic', 'aug', 'pop')[scheme], 'legacy' if fmt == w.FMT_LEGACY else 'modern') for sg, scheme, fmt in COMBOS]


@pytest.mark.parametrize('sg,scheme,fmt', COMBOS, ids=IDS)
def test_kinds_and_expected_statuses(sg, scheme, fmt):
    """every kind exists for every pool triple, the statuses the issue's table fixes are what the oracle gives (asserted while the
    table is built), the pool holds both y-sign bits (asserted while it is built) and all nine message lengths, and the kinds
    whose status is left to the oracle fail to decode"""
    cs = w.cases(sg, scheme, fmt)
    ks = w.kinds(fmt)
    assert len(cs) == len(ks) * w.POOL and len(set(ks)) == len(ks)
    assert sorted(len(t[2]) for t in w.pool(sg, scheme)) == sorted(w.MSG_LENS)
    assert len({t[0] for t in w.pool(sg, scheme)}) == w.POOL and len({t[1] for t in w.pool(sg, scheme)}) == w.POOL
    C = w.IMPLS[sg]
    for (kind, j), (pkb, sigb, msg, want) in cs.items():
        assert len(pkb) == C.PK_BYTES and len(sigb) == C.SIG_BYTES
        assert want in (0, 1, 2, 3, 7, 8) and (want != 8 or fmt == w.FMT_LEGACY)
    fk = w.fail_kinds(sg, scheme, fmt)
    assert set(fk) == set(ks) - set(list(w.KIND_TABLE)[:9])                     # everything crafted is refused by the decoder
    if fmt == w.FMT_LEGACY:
        # two different failures on one item: the key's code wins, in both orders
        assert {cs['pk8_sig7', j][3] for j in range(w.POOL)} == {8} and {cs['pk7_sig8', j][3] for j in range(w.POOL)} == {7}
        for j in range(w.POOL):
            pkb, sigb, _, _ = cs['pk8_sig7', j]
            assert w.decode(C.PK_BYTES, pkb, fmt)[0] == 8 and w.decode(C.SIG_BYTES, sigb, fmt)[0] == 7
            pkb, sigb, _, _ = cs['pk7_sig8', j]
            assert w.decode(C.PK_BYTES, pkb, fmt)[0] == 7 and w.decode(C.SIG_BYTES, sigb, fmt)[0] == 8
    for j in range(w.POOL):                                                     # decode comes before the identity checks
        pkb, sigb, _, want = cs['pk_inf_sig_bad', j]
        assert w.decode(C.PK_BYTES, pkb, fmt) == (0, None) and want == w.decode(C.SIG_BYTES, sigb, fmt)[0] == 7
        pkb, sigb, _, want = cs['pk_inf_sig_hdr', j]
        assert want == w.decode(C.SIG_BYTES, sigb, fmt)[0] and want in w.DECODE_FAIL


def test_layout_roles_every_size():
    """the layout rule alone (no oracle): for every n from 64 to 1,300 and every size the GPU tests use, every pinned site belongs
    to an adjacent (undecodable, valid) pair, items 0 and n - 1 are undecodable, and the shares hold"""
    sizes = set(range(64, 1301)) | {n for v in w.SIZES.values() for n in v if n >= 64} | {n for n in w.SIZES_OTHER if n >= 64}
    for n in sorted(sizes):
        r = w.roles(n)
        w.check_roles(n, r)
        assert {0, n - 1, 31, 32} <= set(w.pinned_sites(n))
        assert 3 * r.count('V') >= n and 3 * r.count('F') >= n and r.count('O') >= 8, n
    assert w.pinned_sites(300) == [0, 31, 32, 63, 64, 95, 96, 127, 128, 159, 160, 191, 192, 223, 224, 255, 256, 299]
    assert w.pinned_sites(4097)[-4:] == [3967, 3968, 4095, 4096]       # both ends of the last full 128-item block


@pytest.mark.parametrize('sg,scheme,fmt', COMBOS, ids=IDS)
def test_batch_conditions(sg, scheme, fmt):
    """the conditions of a cycled batch, on the oracle's expected statuses: every kind, every status, a third valid, a third
    undecodable, an undecodable item next to a valid one at every pinned site; and the two special layouts"""
    ks = set(w.kinds(fmt))
    want_st = {0, 1, 2, 3, 7} | ({8} if fmt == w.FMT_LEGACY else set())
    sizes = [n for n in (w.SIZES[sg] if scheme == ref.POP else w.SIZES_THIN) + w.SIZES_OTHER[:-1] if n >= 64]
    for n in sizes:
        for seed in (0, 5):
            pks, sigs, msgs, st, names = w.build_batch(sg, scheme, fmt, n, seed)
            assert len(pks) == len(sigs) == len(msgs) == len(st) == n
            assert set(names) == ks, (n, ks - set(names))
            assert set(st) == want_st, n
            nfail = sum(s in w.DECODE_FAIL for s in st)
            assert 3 * st.count(0) >= n and 3 * nfail >= n, (n, st.count(0), nfail)
            assert st[0] in w.DECODE_FAIL and st[1] == 0 and st[n - 1] in w.DECODE_FAIL and st[n - 2] == 0
            for s in w.pinned_sites(n):
                near = [st[p] for p in (s - 1, s + 1) if 0 <= p < n]
                assert (st[s] in w.DECODE_FAIL and 0 in near) or (st[s] == 0 and any(x in w.DECODE_FAIL for x in near)), (n, s)
    # below 64 items: a prefix of the kind list rotated by the seed; all rotations of one item cover every kind
    order = w.kinds(fmt)
    assert [w.build_batch(sg, scheme, fmt, 1, s)[4][0] for s in range(len(order))] == list(order)
    assert w.build_batch(sg, scheme, fmt, 33, 4)[4] == [order[(4 + i) % len(order)] for i in range(33)]
    for n in (40, 600, 5000):
        st = w.build_batch(sg, scheme, fmt, n, 3, 'all_fail')[3]
        assert len(st) == n and all(s in w.DECODE_FAIL for s in st) and (fmt != w.FMT_LEGACY or {7, 8} == set(st))
        st = w.build_batch(sg, scheme, fmt, n, 3, 'all_but_one')[3]
        assert st.count(0) == 1 and sum(s in w.DECODE_FAIL for s in st) == n - 1
        assert len({w.build_batch(sg, scheme, fmt, n, s, 'all_but_one')[3].index(0) for s in range(8)}) >= 4       # the survivor moves


def test_scan_raises_instead_of_skipping(monkeypatch):
    """a scan that finds nothing within its bound raises: no kind can drop out silently"""
    start = w.pool(2, ref.POP)[0][0]
    assert w.decode(48, w.scan(48, start, 'offcurve'), w.FMT_COMPRESSED)[0] == 7
    monkeypatch.setattr(w, 'SCAN', 0)
    w.scan.cache_clear()
    try:
        for want in ('offcurve', 'offsub'):
            with pytest.raises(RuntimeError):
                w.scan(48, start, want)
    finally:
        w.scan.cache_clear()


def test_reference_vectors_and_oracle_spellings():
    """the reference's C++ vectors (tests/golden/ref_kats.json), as modern and as legacy bytes, are status 0 for the oracle; and
    for the 48-byte keys and 96-byte signatures of Bls12381G2Impl the header rules spelt out in wire_cases.decode give what the
    oracle's restatement of PublicKey / Signature::from_bytes_with_mode gives, on every crafted encoding"""
    k = json.load(open(os.path.join(util.ROOT, 'tests', 'golden', 'ref_kats.json')))['cpp']
    msg = bytes.fromhex(k['message'])
    for ph, sh in zip(k['pk'], k['sig']):
        pkb, sigb = bytes.fromhex(ph), bytes.fromhex(sh)
        assert w.expected_status(2, ref.BASIC, w.FMT_COMPRESSED, pkb, sigb, msg) == 0
        assert w.expected_status(2, ref.BASIC, w.FMT_LEGACY, ref.modern_to_legacy(pkb), ref.modern_to_legacy(sigb), msg) == 0
        assert w.expected_status(2, ref.BASIC, w.FMT_COMPRESSED, pkb, sigb, msg + b'!') == 1
    seen = 0
    for fmt in FMTS:
        for nbytes, blobs in _blobs(2, ref.POP, fmt).items():
            for b in blobs:
                assert w.decode_via_ref(nbytes, b, fmt) == w.decode(nbytes, b, fmt)[0], (fmt, b.hex())
                seen += 1
    assert seen >= 2 * 10 * w.POOL


def _blobs(sg, scheme, fmt):
    """{width: the distinct key / signature encodings of the kind list}"""
    C = w.IMPLS[sg]
    out = {C.PK_BYTES: set(), C.SIG_BYTES: set()}
    for pkb, sigb, _, _ in w.cases(sg, scheme, fmt).values():
        out[C.PK_BYTES].add(pkb)
        out[C.SIG_BYTES].add(sigb)
    return {k: sorted(v) for k, v in out.items()}


@pytest.mark.parametrize('sg', [1, 2])
@pytest.mark.parametrize('fmt', FMTS, ids=['modern', 'legacy'])
def test_hostsim_decompress_statuses(hs, sg, fmt):
    """the device's g1_decompress / g2_decompress compiled for the host (tests/hostsim): every key and every signature encoding of
    the kind list gives the oracle's decode status (0 / 7 / 8), and what decodes re-compresses to the oracle's modern bytes"""
    C = w.IMPLS[sg]
    n = {0: 0, 7: 0, 8: 0}
    for nbytes, blobs in _blobs(sg, ref.POP, fmt).items():
        comp = C.pk_to_bytes if nbytes == C.PK_BYTES else C.sig_to_bytes
        for b in blobs:
            want, pt = w.decode(nbytes, b, fmt)
            out = ctypes.create_string_buffer(nbytes)
            rc = hs.hs_decompress(nbytes // 48, b, int(fmt == w.FMT_LEGACY), out)
            assert rc == want, (nbytes, fmt, b.hex(), rc, want)
            if rc == 0:
                assert out.raw == comp(pt), b.hex()
            n[rc] += 1
    assert n[0] >= 4 * w.POOL and n[7] >= 4 * w.POOL and (n[8] >= 6 * w.POOL) == (fmt == w.FMT_LEGACY), n
