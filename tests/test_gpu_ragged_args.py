"""The ragged arguments (n + 1 offsets over a flat array) of the batched entry points, by value and over a registered key set: what
the host checks on the offsets it reads, and the text of the error it leaves in blsgpu_last_error.  Every error case returns before a
kernel is launched; the buffers behind the offsets are zero-filled dummies that nothing reads."""
import ctypes
import random

import pytest

import multi_batch_cases
import secure_batch_cases

pytestmark = pytest.mark.gpu

E_ARG = -3
U64P = ctypes.POINTER(ctypes.c_uint64)
Z = (ctypes.c_uint8 * 4096)()               # every input the offsets would index
OUT = (ctypes.c_uint8 * 4096)()             # points / frames out
RANGE = (ctypes.c_uint64 * 8)()
IDX = (ctypes.c_uint32 * 8)()               # positions in the key set of the indexed entry points
KEYSETS = {}                                # sig_group -> a two-key set (the fixture below)


def _combine(lib, sg, n, o, st):
    return lib.blsgpu_combine_shares(sg, Z, Z, None, o['set_offsets'], n, 0, OUT, st)


def _share_verify(lib, sg, n, o, st):
    return lib.blsgpu_signcrypt_share_verify_batch(sg, 0, Z, Z, Z, o['v_offsets'], n, Z, Z, o['share_offsets'], 0, st)


def _open(lib, sg, n, o, st):
    return lib.blsgpu_signcrypt_open_batch(sg, 0, Z, Z, Z, o['v_offsets'], n, Z, Z, o['share_offsets'], 0, OUT, RANGE, st)


def _secure(lib, sg, n, o, st, ser_format=0):
    return lib.blsgpu_verify_secure_batch(sg, 0, Z, o['key_offsets'], n, Z, Z, o['msg_offsets'], ser_format, 0, st)


def _aggregate(lib, sg, n, o, st):
    return lib.blsgpu_aggregate_verify_batch(sg, 0, Z, Z, o['msg_offsets'], o['set_offsets'], n, Z, 0, st, None)


def _multi(lib, sg, n, o, st):
    return lib.blsgpu_multi_verify_batch(sg, 0, Z, o['key_offsets'], n, Z, Z, o['msg_offsets'], 0, st)


def _multi_indexed(lib, sg, n, o, st):
    return lib.blsgpu_multi_verify_indexed_batch(0, KEYSETS[sg].handle, IDX, o['key_offsets'], n, Z, Z, o['msg_offsets'], 0, st)


def _secure_indexed(lib, sg, n, o, st, ser_format=0):
    return lib.blsgpu_verify_secure_indexed_batch(0, KEYSETS[sg].handle, IDX, o['key_offsets'], n, Z, Z, o['msg_offsets'], ser_format, 0, st)


def _sum_indexed(lib, sg, n, o, st):
    return lib.blsgpu_sum_indexed_batch(KEYSETS[sg].handle, IDX, o['offsets'], n, OUT)


def _aggregate_secure(lib, sg, n, o, st, ser_format=0):
    return lib.blsgpu_aggregate_secure_batch(sg, Z, Z, o['key_offsets'], n, ser_format, 0, OUT, st)


# entry point -> (call, every offsets argument in the order the host reads them, those it checks for "[0] must be 0")
ENTRIES = {
    'combine_shares': (_combine, ['set_offsets'], ['set_offsets']),
    'signcrypt_share_verify_batch': (_share_verify, ['v_offsets', 'share_offsets'], ['v_offsets', 'share_offsets']),
    'signcrypt_open_batch': (_open, ['v_offsets', 'share_offsets'], ['v_offsets', 'share_offsets']),
    'verify_secure_batch': (_secure, ['key_offsets', 'msg_offsets'], ['key_offsets']),
    # the per-pair msg_offsets of the aggregate batch are an argument, but the host reads one total from them and checks nothing
    'aggregate_verify_batch': (_aggregate, ['set_offsets'], ['set_offsets']),
    'multi_verify_batch': (_multi, ['key_offsets', 'msg_offsets'], ['key_offsets']),
    'multi_verify_indexed_batch': (_multi_indexed, ['key_offsets', 'msg_offsets'], ['key_offsets']),
    'verify_secure_indexed_batch': (_secure_indexed, ['key_offsets', 'msg_offsets'], ['key_offsets']),
    'sum_indexed_batch': (_sum_indexed, ['offsets'], ['offsets']),
}
# the secure calls, for their ser_format argument (the secure aggregation is no entry of the tables above)
SECURE = {'verify_secure_batch': _secure, 'verify_secure_indexed_batch': _secure_indexed, 'aggregate_secure_batch': _aggregate_secure}
ALL_ARGS = {'aggregate_verify_batch': ['set_offsets', 'msg_offsets']}
READ = [(e, a) for e, (_, args, _) in ENTRIES.items() for a in args]
ZERO_CHECKED = [(e, a) for e, (_, _, args) in ENTRIES.items() for a in args]
ids = lambda pairs: ['%s-%s' % p for p in pairs]


@pytest.fixture(scope='module', autouse=True)
def keysets(api):
    """one set of two keys per signature group, for the indexed entry points"""
    for sg in (1, 2):
        KEYSETS[sg] = api.KeySet.create(sg, api.serialize(3 - sg, api.sign_batch(sg, 0, [5, 6], [b'', b''])[0]))
    yield
    for ks in KEYSETS.values():
        ks.close()
    KEYSETS.clear()


class Offsets:
    """Offset arrays on the host or on the device, kept alive for the call."""

    def __init__(self, where):
        self.where, self.keep = where, []

    def __call__(self, values):
        if self.where == 'host':
            a = (ctypes.c_uint64 * len(values))(*values)
            self.keep.append(a)
            return ctypes.cast(a, U64P)
        import torch
        t = torch.tensor(values, dtype=torch.int64, device='cuda:0')
        torch.cuda.synchronize()
        self.keep.append(t)
        return ctypes.cast(ctypes.c_void_p(t.data_ptr()), U64P)


def run(api, entry, sg, n, given, where='host', **kw):
    """One call with `given` ({argument: offsets list or None}) and valid all-zero offsets for the entry's other arguments; kw goes
    to the call.  Returns (return code, last error text, status buffer)."""
    lib = api.init()
    call, args = (SECURE[entry], ['key_offsets', 'msg_offsets']) if entry in SECURE else ENTRIES[entry][:2]
    mk = Offsets(where)
    o = {a: mk([0] * (n + 1)) for a in ALL_ARGS.get(entry, args)}
    for a, v in given.items():
        o[a] = None if v is None else mk(v)
    st = (ctypes.c_int32 * 4)(-99, -99, -99, -99)
    rc = call(lib, sg, n, o, st, **kw)
    buf = ctypes.create_string_buffer(1024)
    lib.blsgpu_last_error(buf, 1024)
    return rc, buf.value.decode(), list(st)


@pytest.mark.parametrize('where', ['host', 'device'])
@pytest.mark.parametrize('sg', [1, 2])
@pytest.mark.parametrize('entry,arg', ZERO_CHECKED, ids=ids(ZERO_CHECKED))
def test_first_offset_not_zero(api, entry, arg, sg, where):
    rc, err, st = run(api, entry, sg, 2, {arg: [1, 1, 2]}, where)
    assert (rc, err) == (E_ARG, arg + '[0] must be 0')
    assert st == [-99] * 4


@pytest.mark.parametrize('where', ['host', 'device'])
@pytest.mark.parametrize('sg', [1, 2])
@pytest.mark.parametrize('entry,arg', READ, ids=ids(READ))
def test_decreasing_offsets(api, entry, arg, sg, where):
    rc, err, st = run(api, entry, sg, 2, {arg: [0, 2, 1]}, where)
    assert (rc, err) == (E_ARG, arg + ' must not decrease')
    assert st == [-99] * 4


@pytest.mark.parametrize('sg', [1, 2])
@pytest.mark.parametrize('entry,arg', READ, ids=ids(READ))
def test_null_offsets(api, entry, arg, sg):
    rc, err, st = run(api, entry, sg, 2, {arg: None})
    assert rc == E_ARG and err
    assert st == [-99] * 4


@pytest.mark.parametrize('sg', [1, 2])
@pytest.mark.parametrize('entry', list(ENTRIES))
def test_no_sets(api, entry, sg):
    """n = 0 with the one offset that is left: success, and no status is written."""
    rc, _, st = run(api, entry, sg, 0, {})
    assert rc == 0
    assert st == [-99] * 4


@pytest.mark.parametrize('sg,ser_format,text', [
    (1, 2, 'ser_format must be 0 (Modern) or 1 (Legacy)'), (2, 2, 'ser_format must be 0 (Modern) or 1 (Legacy)'),
    (1, 1, 'Legacy serialization exists only for Bls12381G2Impl (48-byte keys), reference src/signature.rs:201-204')])
@pytest.mark.parametrize('entry', list(SECURE))
def test_ser_format(api, entry, sg, ser_format, text):
    """The serialisation argument of the secure calls, over valid offsets: a value that is none, and Legacy with 96-byte keys."""
    rc, err, st = run(api, entry, sg, 2, {}, ser_format=ser_format)
    assert (rc, err) == (E_ARG, text)
    assert st == [-99] * 4


@pytest.mark.parametrize('sg', [1, 2])
@pytest.mark.parametrize('entry', ['verify_secure_batch', 'multi_verify_batch'])
def test_per_set_msg_offsets_need_not_start_at_zero(api, entry, sg):
    """The per-set msg_offsets of the secure and multi batches are only checked for order (a set's message is msgs + msg_offsets[s]).
    Two real sets, the second with a wrong message: offsets that start at 1 over a buffer with one byte in front give the statuses
    of offsets that start at 0; so do the offsets [1, 1, 2] themselves, against [0, 0, 1] over the buffer without its first byte."""
    lib = api.init()
    if entry == 'verify_secure_batch':
        sets = secure_batch_cases.valid_sets(api, sg, api.BASIC, [2, 3], random.Random(7 + sg))
        whole = lambda s: api.verify_secure_batch(sg, api.BASIC, s)
        raw = lambda mo, mb, st: lib.blsgpu_verify_secure_batch(sg, api.BASIC, pkb, koffs, 2, sgb, mb, mo, api.MODERN, api.FMT_RAW_PROJ, st)
    else:
        sets = multi_batch_cases.valid_sets(api, sg, api.BASIC, [2, 3], random.Random(9 + sg))
        whole = lambda s: api.multi_verify_batch(sg, api.BASIC, s)
        raw = lambda mo, mb, st: lib.blsgpu_multi_verify_batch(sg, api.BASIC, pkb, koffs, 2, sgb, mb, mo, api.FMT_RAW_PROJ, st)
    sets = [sets[0][:3], (sets[1][0], sets[1][1], sets[1][2] + b'!')]
    want = whole(sets)
    assert want == [api.OK, api.INVALID_SIGNATURE]
    pkb = api._ptr(b''.join(p for pks, _, _ in sets for p in pks))
    sgb = api._ptr(b''.join(sig for _, sig, _ in sets))
    koffs = ctypes.cast((ctypes.c_uint64 * 3)(0, 2, 5), ctypes.c_void_p)
    m0, m1 = sets[0][2], sets[1][2]

    def statuses(moffs, blob):
        st = (ctypes.c_int32 * 2)(-99, -99)
        mo = (ctypes.c_uint64 * 3)(*moffs)
        api._check(raw(ctypes.cast(mo, ctypes.c_void_p), api._ptr(blob), ctypes.cast(st, ctypes.c_void_p)))
        return list(st)

    assert statuses([1, 1 + len(m0), 1 + len(m0) + len(m1)], b'\xa5' + m0 + m1) == want
    blob = b'\xa5' + m0
    assert statuses([1, 1, 2], blob) == statuses([0, 0, 1], blob[1:]) == [api.INVALID_SIGNATURE] * 2
