"""tests/pok_timestamp_cases.py on the CPU: the restatement of HashToScalar is the oracle's key generation under the key-generation
salt, and every kind of the case list is what its name says, per orientation, scheme and mode, by the oracle's proof check."""
import hashlib

import pytest

import pok_timestamp_cases as pc
from oracle.py import bls381 as c
from oracle.py import blsful_ref as ref


def test_hash_to_scalar_is_the_oracles_keygen():
    for j in range(6):
        seed = hashlib.sha256(b'pok-seed-%d' % j).digest()[:(32, 1, 31, 33, 64, 0)[j]]
        assert pc.hash_to_scalar(seed, pc.KEYGEN_SALT) == ref.keygen_from_hash(seed)
    assert len(pc.POK_SALT) == 36


def test_timeout_rule():
    f = pc.timeout_status
    assert f(5, 4, None) is None and f(0, pc.U64_MAX, None) is None
    assert f(pc.NOW - pc.TIMEOUT, pc.NOW, pc.TIMEOUT) is None                     # elapsed == timeout passes
    assert f(pc.NOW - pc.TIMEOUT - 1, pc.NOW, pc.TIMEOUT) == pc.INVALID_SIGNATURE
    assert f(pc.NOW + 1, pc.NOW, pc.TIMEOUT) == pc.E_ARG and f(pc.NOW, pc.NOW, 0) is None


@pytest.mark.parametrize('scheme', pc.SCHEMES)
@pytest.mark.parametrize('sg', (1, 2))
def test_kinds_are_what_they_say(sg, scheme):
    C = pc.IMPLS[sg]
    its = pc.items(sg, scheme)
    for kind in pc.KINDS:
        got = tuple(pc.expected(sg, scheme, kind, mode) for mode in ('none', 'timeout'))
        assert got == pc.WANT[kind], (kind, got)
    # the proofs are made for their own t: y = compute_y(U, t) is what the proof check gets
    u, v, pk, t, msg = its['valid']
    y = pc.compute_y(C, u, t)
    assert 0 < y < c.R
    ref.sig_proof_verify(C, u, v, pk, y, msg, C.DST[scheme])
    assert pc.compute_y(C, u, t + 1) != y
    # the kinds the timeout rule decides sit on its edges
    assert its['at_limit'][3] == pc.NOW - pc.TIMEOUT and its['past_limit'][3] == its['at_limit'][3] - 1
    assert its['future_with_timeout'][3] == pc.NOW + 1 and its['t_zero'][3] == 0 and its['t_max'][3] == 2 ** 64 - 1
    assert its['past_limit_u_inf'][0] is None and its['past_limit_u_inf'][1:] == its['past_limit'][1:]


def test_batches_interleave_the_kinds():
    cols, want, names = pc.build_batch(1, ref.POP, 65, 'timeout')
    assert len(want) == 65 and set(names) == set(pc.KINDS) and names[:len(pc.KINDS)] == list(pc.KINDS)
    assert {len(x) for x in cols[0]} == {144} and {len(x) for x in cols[2]} == {288}
    a, _, _ = pc.build_batch(1, ref.POP, 14, 'timeout')
    assert a[0][0] != a[0][13] and pc.KINDS[0] == pc.KINDS[13 % len(pc.KINDS)]     # a repeated item is rendered afresh
    for fmt, w in ((pc.RAW_AFFINE, 96), (pc.COMPRESSED, 48), (pc.LEGACY, 48)):
        cols, _, _ = pc.build_batch(2, ref.BASIC, 14, 'none', fmt=fmt)
        assert {len(x) for x in cols[2]} == {w} and {len(x) for x in cols[0]} == {2 * w}
