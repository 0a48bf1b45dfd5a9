"""The case list of the indexed time-lock call (blsgpu_timecrypt_open_indexed_batch), built from tests/timecrypt_cases.py
timelock_groups(sg) and shared by tests/test_sigset_cases.py (CPU: what the list claims for itself) and tests/test_gpu_sigset.py (the
calls).  Every group's signature -- the undecodable ones on the wire formats and the identity included, and those of the empty groups
-- becomes an ENTRY of a signature set; every item names its entry; the items are shuffled so that no two neighbours share an entry;
two extra items name n and 0xffffffff.  The expected statuses and messages are the by-value list's (timecrypt_cases.expected_item),
plus BLSGPU_E_ARG for the two extra items.  No second oracle: nothing here computes a pairing or opens a frame."""
import random

import timecrypt_cases as tc

E_ARG = -3
NO_ENTRY = 0xffffffff


def shuffled(per_entry):
    """[(entry, item)] from {entry: [items]}: always the entry with the most items left that is not the previous one (ties: the lower
    entry), which leaves no two neighbours on one entry as long as no entry holds more than half of the items, rounded up"""
    left = {k: list(v) for k, v in per_entry.items() if v}
    out, prev = [], None
    while left:
        k = max((k for k in left if k != prev), key=lambda k: (len(left[k]), -k), default=None)
        assert k is not None, 'one entry holds more than half of the items'
        out.append((k, left[k].pop(0)))
        if not left[k]:
            del left[k]
        prev = k
    return out


def render(sg, fmt, seed=0, groups=None):
    """One call under a format -> (entries, entry statuses, items, messages, statuses, names):
      entries   [(signature bytes, scheme tag)] as api.SignatureSet.create takes them
      entry statuses  what creation must report per entry (the decode status on the wire formats, else OK)
      items     [(idx, u, v, w, scheme tag)] as api.timecrypt_open_indexed_batch takes them
    On the raw formats the members that exist as wire bytes only are left out (the items, and the entries of such a signature)."""
    rng = random.Random(53 * fmt + seed)
    wire = fmt in (tc.COMPRESSED, tc.LEGACY)
    groups = tc.timelock_groups(sg) if groups is None else groups
    entries, est, per_entry = [], [], {}
    for g in groups:
        if g['sig_bad'] and not wire:
            continue
        k = len(entries)
        if g['sig_bad']:
            b = tc.bad_wire(sg, g['sig_bad'], fmt)
            est.append(tc.decode_status(sg, b, fmt))
        else:
            b = tc.render_point(sg, g['sig'], fmt, rng)
            est.append(tc.OK)
        entries.append((b, g['scheme']))
        per_entry[k] = [(g, it) for it in g['items'] if wire or not it['u_bad']]
    items, msgs, sts, names = [], [], [], []
    for k, (g, it) in shuffled(per_entry):
        u = tc.bad_wire(3 - sg, it['u_bad'], fmt) if it['u_bad'] else tc.render_point(3 - sg, it['u'], fmt, rng)
        items.append((k, u, it['v'], it['w'], it['scheme']))
        st, m = tc.expected_item(sg, g, it, fmt)
        sts.append(st)
        msgs.append(m)
        names.append(it['name'])
    # the two items that name no entry: a good ciphertext each, one in the middle and one at the end
    good = next(i for i, s in enumerate(sts) if s == tc.OK)
    for at, k in ((len(items) // 2, len(entries)), (len(items) + 1, NO_ENTRY)):
        items.insert(at, (k,) + items[good][1:])
        sts.insert(at, E_ARG)
        msgs.insert(at, None)
        names.insert(at, 'index %d of %d entries' % (k, len(entries)))
    return entries, est, items, msgs, sts, names


def rows_groups(sg):
    """the groups whose signature has usable rows, with the items that exist in every format: no wire-only member, no identity
    signature, no empty group"""
    return [dict(g, items=[it for it in g['items'] if not it['u_bad']]) for g in tc.timelock_groups(sg)
            if not g['sig_bad'] and g['sig'] is not None and g['items']]


def three_groups(sg):
    """three of rows_groups(sg), none with more than half of their items: round trips of two schemes and the signature of another round"""
    g = rows_groups(sg)
    return [g[3], g[4], g[8]]


def tiled(sg, fmt, n, seed=0, groups=None):
    """n items over the entries of rows_groups(sg) (or of `groups`), the shuffled list repeated and cut -> (entries, items, messages,
    statuses)"""
    entries, est, items, msgs, sts, _ = render(sg, fmt, seed, rows_groups(sg) if groups is None else groups)
    keep = [i for i, s in enumerate(sts) if s != E_ARG]
    assert est == [tc.OK] * len(entries) and len(keep) >= 2
    pick = [keep[i % len(keep)] for i in range(n)]
    return entries, [items[i] for i in pick], [msgs[i] for i in pick], [sts[i] for i in pick]
