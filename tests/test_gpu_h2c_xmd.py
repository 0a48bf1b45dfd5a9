"""expand_message_xmd on every hash path, selected by batch size alone (default knobs, no environment switches), at the tag lengths
where its block arithmetic changes, against oracle/c (bo_hash_to_point).

Batch sizes -> kernels (csrc/blsgpu.hip run_hash_group):
  G1   1: k_hash_to_g1_engine      129: k_hash_to_g1_wide            513: k_hash_to_g1 on lane pairs    4097: k_hash_to_g1, one lane
  G2   1: k_hash_to_g2_engine      129: k_hash_to_g2_maps + tail     513: k_hash_to_g2 on lane pairs
The first two of each group run expand_message_xmd_wave, the others expand_message_xmd_words (whole-word messages, with its cached tag
words: TW = 24, tags up to 93 bytes) or the byte-streaming expand_message_xmd (every other message length).  Message i is the same
bytes in every batch, so the paths must also agree index by index.

Tag lengths: 1; 21 / 22 / 23 where 34 + len crosses the first SHA block's room for the padding, 85 / 86, 149 / 150, 213 / 214 the later
blocks; 93 / 94 / 95 the edge of the tag cache; 43 the scheme tags' length; 254 / 255 the longest plain tags; 256 the first that is
hashed down (RFC 9380 5.3.3).  Message lengths cycle through 0, 1, 3, 4, 31, 32, 33, 55, 56, 63, 64, 65, 119, 120, 127, 128, 129, 200,
257 and the messages are concatenated raggedly, so whole-word messages start at unaligned addresses (the be32_at branch of
expand_message_xmd_words); a second batch has every message 32 bytes long (the aligned branch).

Expected values: oracle/c for every item up to n = 513; at n = 4097 for 200 sampled items, the first 513 by agreement with the
smaller batch.  Comparison: the RAW_PROJ output normalised with Python integers and compressed by oracle/py, byte for byte."""
import ctypes
import random

import pytest

import h2c_cases as hc
import util
from oracle.py import bls381 as c

pytestmark = pytest.mark.gpu

TAG_LENS = (1, 21, 22, 23, 43, 85, 86, 93, 94, 95, 149, 150, 213, 214, 254, 255, 256)
MSG_LENS = (0, 1, 3, 4, 31, 32, 33, 55, 56, 63, 64, 65, 119, 120, 127, 128, 129, 200, 257)
SIZES = {1: (1, 129, 513, 4097), 2: (1, 129, 513)}
N_MAX = 4097
SAMPLES = 200


def messages(kind):
    rng = random.Random(0x786d64 + (kind == 'aligned'))
    return [rng.randbytes(32 if kind == 'aligned' else MSG_LENS[i % len(MSG_LENS)]) for i in range(N_MAX)]


MSGS = {kind: messages(kind) for kind in ('ragged', 'aligned')}


def compressed(group, raw):
    pt = hc.normalise(group, raw)
    return c.g1_compress(pt) if group == 1 else c.g2_compress(pt)


def expected(bo, group, msg, dst):
    out = ctypes.create_string_buffer(48 * group)
    bo.bo_hash_to_point(group, msg, len(msg), dst, len(dst), out)
    return out.raw


@pytest.mark.parametrize('tag_len', TAG_LENS)
def test_expansion_on_every_path(api, tag_len):
    bo = util.load_c_oracle()
    rng = random.Random(1000 + tag_len)
    dst = rng.randbytes(tag_len)
    sampled = sorted(rng.sample(range(513, N_MAX), SAMPLES - 1) + [N_MAX - 1])
    for group in (1, 2):
        for kind in ('ragged', 'aligned'):
            msgs = MSGS[kind]
            want = [expected(bo, group, m, dst) for m in msgs[:513]]
            sizes = SIZES[group] if kind == 'ragged' else SIZES[group][2:]      # the aligned branch exists in expand_message_xmd_words only
            prev = None
            for n in sizes:
                got = [compressed(group, o) for o in api.hash_to_point(group, msgs[:n], dst)]
                assert len(got) == n
                for i in range(min(n, 513)):
                    assert got[i] == want[i], 'G%d, tag of %d bytes, %s messages, n = %d: item %d (%d bytes)' % (group, tag_len, kind, n, i, len(msgs[i]))
                if n > 513:
                    assert got[:513] == prev[:513]
                    for i in sampled:
                        assert got[i] == expected(bo, group, msgs[i], dst), 'G%d, tag of %d bytes, %s messages, n = %d: item %d' % (group, tag_len, kind, n, i)
                prev = got
