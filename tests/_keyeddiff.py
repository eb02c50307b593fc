"""The plain-Python restatement the keyed-diff tests compare with (tests/test_keyed_diff.py,
test_keyed_diff_cpu.py): dicts and lists, nothing here calls the library.

The reference (repositories/diffs/join_diff.rs) full-joins the two hashed frames on the key hash (:290),
labels every joined row through `test_function` (:458-484), filters the unchanged ones out (:88-92),
counts the rest (:434-456) and counts the rows of duplicated keys on each side (core/df/tabular.rs:263-271).
Restated from those lines, not pinned by a run of polars:

    joined rows   every (l, r) with equal key digests (the whole cross product when a key repeats),
                  (l, None) for a left row without a partner, (None, r) for a right row without one
    status        1. left absent or the left row's keys[0] cell null        -> added
                  2. else right absent or the right row's keys[0] cell null -> removed
                  3. else no targets on either side                          -> unchanged
                  4. else the target digests differ (None == None, None != any digest) -> modified
                  5. else                                                    -> unchanged
    order         the left rows ascending, each followed by its pairs (right rows ascending) or its one
                  (l, None); then the right-only rows ascending (the project's canonical order)
"""
UNCHANGED, ADDED, REMOVED, MODIFIED = 0, 1, 2, 3


def status_of(l, r, left_targets, right_targets, left_valid, right_valid):
    if l is None or (left_valid is not None and not left_valid[l]):
        return ADDED
    if r is None or (right_valid is not None and not right_valid[r]):
        return REMOVED
    if left_targets is None and right_targets is None:
        return UNCHANGED
    a = None if left_targets is None else left_targets[l]
    b = None if right_targets is None else right_targets[r]
    return MODIFIED if a != b else UNCHANGED


def keyed_diff(left_keys, right_keys, left_targets=None, right_targets=None, left_valid=None, right_valid=None,
               keep_unchanged=False):
    """left_keys / right_keys: lists of hashable key digests; *_targets: lists of digests or None (the null
    column); *_valid: lists of booleans (the validity of keys[0]) or None. Returns (pairs, counts, dupes):
    the emitted (l, r, status) in the canonical order with None for an absent side, {status: joined rows}
    over ALL joined rows, and (dupes left, dupes right)."""
    by_key = {}
    for r, k in enumerate(right_keys):
        by_key.setdefault(k, []).append(r)      # ascending
    left_seen = {}
    for k in left_keys:
        left_seen[k] = left_seen.get(k, 0) + 1
    joined = []
    for l, k in enumerate(left_keys):
        partners = by_key.get(k)
        if partners is None:
            joined.append((l, None))
        else:
            joined.extend((l, r) for r in partners)
    joined.extend((None, r) for r, k in enumerate(right_keys) if k not in left_seen)
    counts = {UNCHANGED: 0, ADDED: 0, REMOVED: 0, MODIFIED: 0}
    pairs = []
    for l, r in joined:
        s = status_of(l, r, left_targets, right_targets, left_valid, right_valid)
        counts[s] += 1
        if s != UNCHANGED or keep_unchanged:
            pairs.append((l, r, s))
    dupes = (sum(1 for k in left_keys if left_seen[k] > 1), sum(1 for k in right_keys if len(by_key[k]) > 1))
    return pairs, counts, dupes
