"""numpy model of smx_recon_compact (include/smx.h), used by the compaction tests on both sides: the GPU result is
compared with it, and the oracle's state is compacted with it in place.  Test infrastructure."""
import numpy as np

INVALID = 0xFFFFFFFF
LINK_ROWS = slice(19, 23)


def compact_rows(rows, n):
    """rows: [25, >= n] float32 in the reference's row layout.  Returns (new_rows [25, k], old_to_new [n] uint32,
    links_dropped): slot i is kept iff !(RadiusSquared < 0); kept slots keep their order; links go through the map,
    a link to a removed slot becomes INVALID; links_dropped counts the valid links of removed slots plus the links of
    kept slots into removed ones."""
    rows = np.asarray(rows, np.float32)
    keep = ~(rows[7, :n] < 0)
    k = int(keep.sum())
    old_to_new = np.full(n, INVALID, np.uint32)
    old_to_new[keep] = np.arange(k, dtype=np.uint32)
    links = rows[LINK_ROWS, :n].view(np.uint32)
    valid = links != INVALID
    mapped = np.full(links.shape, INVALID, np.uint32)
    inside = valid & (links < n)
    mapped[inside] = old_to_new[links[inside]]
    dropped = int(valid[:, ~keep].sum()) + int((valid[:, keep] & (mapped[:, keep] == INVALID)).sum())
    new = np.ascontiguousarray(rows[:, :n][:, keep])
    new[LINK_ROWS] = mapped[:, keep].view(np.float32)
    return new, old_to_new, dropped


def compact_oracle(recon):
    """Compacts the oracle's state in place (what smx_recon_compact does to the GPU map); returns (old_to_new,
    links_dropped).  The rows above the new count keep what they held, as on the GPU."""
    n = recon.surfels_size
    S = recon.surfels()
    new, old_to_new, dropped = compact_rows(S, n)
    S[:, :new.shape[1]] = new
    recon.set_counts(new.shape[1], 0)
    return old_to_new, dropped


def clear_zombie_links(rows, n):
    """Sets the links of the merged slots in [0, n) to INVALID (in place): compaction then drops no link held by a
    removed slot."""
    merged = rows[7, :n] < 0
    links = rows[LINK_ROWS].view(np.uint32)
    links[:, :n][:, merged] = INVALID


def relabel(rows, n, old_to_new, n_old):
    """The rows [0, n) of an UNCOMPACTED map, in the slot order of the compacted one: slot i < n_old goes to
    old_to_new[i] (removed slots are dropped), a slot i >= n_old created later goes to i - (removed count); links go
    through the same map.  Returns [25, n - removed]."""
    removed = n_old - int((old_to_new != INVALID).sum())
    full = np.concatenate([old_to_new, np.arange(n_old, n, dtype=np.uint32) - np.uint32(removed)]).astype(np.uint32)
    keep = full != INVALID
    out = np.zeros((rows.shape[0], n - removed), np.float32)
    out[:, full[keep]] = rows[:, :n][:, keep]
    links = out[LINK_ROWS].view(np.uint32)
    valid = links != INVALID
    links[valid] = full[links[valid]]
    return out
