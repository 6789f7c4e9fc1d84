"""The id planes in numpy: csrc/er_ids.h restated, so that what er_render_ids leaves on the device (and er_debug_id_rank on the host) can
be held against it word for word.

A pixel's ids of one kind are the ids of its rays that HIT (misses are not in the list).  Its slots are the distinct ids ordered by
(count descending, id ascending as unsigned), the first ID_SLOTS of them; unused slots are (ID_NONE, 0).  ID_NONE -- a hit on geometry
in no object -- is an id like any other and, being the largest unsigned value, last among equal counts."""
import numpy as np

ID_NONE = 0xFFFFFFFF
ID_SLOTS = 4


def rank(ids):
    """(slot ids uint32[ID_SLOTS], slot counts uint32[ID_SLOTS], distinct) of one pixel's hit ids."""
    a = np.asarray(ids, np.uint32).reshape(-1)
    out_id, out_count = np.full(ID_SLOTS, ID_NONE, np.uint32), np.zeros(ID_SLOTS, np.uint32)
    if a.size == 0:
        return out_id, out_count, 0
    u, c = np.unique(a, return_counts=True)          # ascending ids
    order = np.lexsort((u, -c.astype(np.int64)))     # count descending, then id ascending
    k = min(ID_SLOTS, u.size)
    out_id[:k], out_count[:k] = u[order[:k]], c[order[:k]]
    return out_id, out_count, int(u.size)


def tie_at_the_cut(ids):
    """the fourth and the fifth id of the ranking have the same count: only the id order decides which one is kept"""
    a = np.asarray(ids, np.uint32).reshape(-1)
    c = np.sort(np.unique(a, return_counts=True)[1])[::-1]
    return c.size > ID_SLOTS and c[ID_SLOTS - 1] == c[ID_SLOTS]


def planes(hit_ids, hit):
    """hit_ids uint32[P, n], hit bool[P, n] (ray k of pixel p hit) -> (ids uint32[P, ID_SLOTS], counts the same, overflow pixels)."""
    hit_ids, hit = np.asarray(hit_ids, np.uint32), np.asarray(hit, bool)
    ids, counts = np.full((len(hit_ids), ID_SLOTS), ID_NONE, np.uint32), np.zeros((len(hit_ids), ID_SLOTS), np.uint32)
    overflow = 0
    for p in range(len(hit_ids)):
        ids[p], counts[p], distinct = rank(hit_ids[p][hit[p]])
        overflow += distinct > ID_SLOTS
    return ids, counts, overflow


def object_of(tri_count, objects):
    """tri -> object index of a list of id arrays (ID_NONE: in no object)"""
    m = np.full(tri_count, ID_NONE, np.uint32)
    for o, t in enumerate(objects):
        m[np.asarray(t, np.int64)] = o
    return m


def matte(ids, counts, members, n):
    """er_id_matte: float32(sum of the counts of the slots whose id is a member) / float32(n), per pixel"""
    inside = np.isin(ids, np.asarray(members, np.uint32)) & (counts > 0)
    return (np.where(inside, counts, 0).sum(-1).astype(np.float32) / np.float32(n)).astype(np.float32)


def rect(ids, counts, x0, y0, x1, y1):
    """er_pick_rect on (H, W, ID_SLOTS) planes: the distinct ids with a count in the half-open rectangle, ascending"""
    i, c = ids[y0:y1, x0:x1], counts[y0:y1, x0:x1]
    return np.unique(i[c > 0]).astype(np.uint32)
