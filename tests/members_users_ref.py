"""Who owns row r of X under a session's frame geometry -- the numpy statement
the users form of the members' predict_proba is tested against
(tests/test_members_users.py pins it to a pandas groupby).

Stacked song g owns the rows ``frame_perm[frame_offsets[g]:frame_offsets[g+1]]``
(or that range itself without a ``frame_perm``); user u owns the stacked songs
``item_offsets[u]:item_offsets[u+1]``."""
import numpy as np


def row_owners(item_offsets, frame_offsets, frame_perm, F):
    """(user [F], song [F]) of every row of X, -1 where no song owns the row.
    A position whose row is outside [0, F) names no row."""
    item_offsets = np.asarray(item_offsets, np.int64)
    frame_offsets = np.asarray(frame_offsets, np.int64)
    user, song = np.full(F, -1, np.int64), np.full(F, -1, np.int64)
    for u in range(len(item_offsets) - 1):
        for g in range(item_offsets[u], item_offsets[u + 1]):
            pos = np.arange(frame_offsets[g], frame_offsets[g + 1])
            rows = pos if frame_perm is None else np.asarray(frame_perm, np.int64)[pos]
            rows = rows[(rows >= 0) & (rows < F)]
            user[rows], song[rows] = u, g
    return user, song


def excl_words(songs, T):
    """The exclusion bitmap over T stacked songs (int32 words, bit g of word g // 32) with `songs` set."""
    w = np.zeros(max((T + 31) // 32, 1), np.uint32)
    for g in songs:
        w[g >> 5] |= np.uint32(1) << np.uint32(g & 31)
    return w.view(np.int32)
