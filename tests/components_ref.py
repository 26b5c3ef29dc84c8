"""The rule of segdino3d_amd/components.py restated on the host, in numpy and a plain union-find: what csrc/components.hip must EQUAL,
bit for bit.  tests/test_components_ref.py pins this file itself against brute-force reachability and hand-computed cases.

`components_ref(n, links, source, coords=None, ...)` returns everything the device returns: labels, the per-component tables trimmed
to K, keep, the cleaned nodes / links / maps, and the eight counters as a dict."""
from types import SimpleNamespace

import numpy as np

F32 = np.float32
LIMIT = F32(16384.0)                                     # |c| < 2^14
INFO = ("components", "kept", "nodes", "links", "bad_nodes", "bad_links", "isolated", "unsettled")


def float_key(x):
    """The integer key of fp32 bits: b ^ 0x80000000 for b >= 0, ~b otherwise, as uint32; its order is the floats' order with -0 < +0."""
    b = np.ascontiguousarray(x, F32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)


def link_ends(links, source, n):
    """-> (ends int64 [L, W], skipped bool [L]): the links of a source one per row.  A table [n, k] becomes the n k pairs (i, entry) in
    row-major order, and an entry of -1 is an empty slot."""
    links = np.asarray(links, np.int32)
    if source == "faces":
        assert links.ndim == 2 and links.shape[1] == 3
        return links.astype(np.int64), np.zeros(len(links), bool)
    if source == "edges":
        assert links.ndim == 2 and links.shape[1] == 2
        return links.astype(np.int64), np.zeros(len(links), bool)
    assert source == "table" and links.ndim == 2 and links.shape[0] == n
    k = links.shape[1]
    ends = np.stack([np.repeat(np.arange(n, dtype=np.int64), k), links.reshape(-1).astype(np.int64)], axis=1)
    return ends, ends[:, 1] == -1


def components_ref(n, links, source, coords=None, min_nodes=0, min_links=0, min_extent=0.0, keep_largest=0):
    ends, skipped = link_ends(links, source, n)
    L, W = ends.shape
    # 1. good nodes
    if coords is None:
        good = np.ones(n, bool)
        C = 0
    else:
        coords = np.ascontiguousarray(coords, F32)
        assert coords.shape[0] == n and 3 <= coords.shape[1] <= 11
        C = coords.shape[1]
        with np.errstate(invalid="ignore"):
            good = (np.abs(coords) < LIMIT).all(axis=1)                                  # a NaN compares false
    # 2. good links
    inside = ((ends >= 0) & (ends < n)).all(axis=1)
    ok = inside & ~skipped
    if n:
        ok &= good[np.clip(ends, 0, n - 1)].all(axis=1)
    bad_links = int((~ok & ~skipped).sum())
    # 3. components: a plain union-find, the smaller root wins, so a root is the smallest node of its class
    parent = list(range(n))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    touched = np.zeros(n, bool)
    for row in ends[ok].tolist():
        for a, b in zip(row[:-1], row[1:]):
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
        touched[row] = True
    root = np.array([find(i) for i in range(n)], np.int64).reshape(n)
    is_root = good & (root == np.arange(n))
    number = np.cumsum(is_root) - 1                                                      # ascending smallest node
    labels = np.where(good, number[root] if n else 0, -1).astype(np.int32).reshape(n)
    K = int(is_root.sum())
    # 4. per component
    n_nodes = np.bincount(labels[good], minlength=K).astype(np.int32)
    first = ends[ok][:, 0]
    n_links = np.bincount(labels[first], minlength=K).astype(np.int32) if len(first) else np.zeros(K, np.int32)
    box = np.zeros((K, 6), F32)
    extent = np.zeros(K, F32)
    if coords is not None:
        for c in range(K):
            xyz = coords[labels == c][:, :3]
            key = float_key(xyz)
            for a in range(3):
                box[c, 2 * a] = xyz[np.argmin(key[:, a]), a]
                box[c, 2 * a + 1] = xyz[np.argmax(key[:, a]), a]
        d = np.stack([(box[:, 2 * a + 1] - box[:, 2 * a]).astype(F32) for a in range(3)], axis=1) if K else np.zeros((0, 3), F32)
        extent = d.max(axis=1).astype(F32) if K else extent
    # 5. keep
    passing = (n_nodes >= min_nodes) & (n_links >= min_links) & (extent >= F32(min_extent))
    keep = passing.copy()
    if keep_largest > 0:
        order = sorted(np.flatnonzero(passing).tolist(), key=lambda c: (-int(n_links[c]), c))
        keep = np.zeros(K, bool)
        keep[order[:keep_largest]] = True
    # 6. the clean
    node_keep = good & keep[np.clip(labels, 0, None)] if K else np.zeros(n, bool)
    node_map = np.where(node_keep, np.cumsum(node_keep) - 1, -1).astype(np.int32)
    comp_new = (np.cumsum(keep) - 1).astype(np.int32)
    labels_out = comp_new[labels[node_keep]] if K else np.zeros(0, np.int32)
    nodes = coords[node_keep] if coords is not None else None
    link_keep = ok.copy()
    if L:
        link_keep[ok] = node_keep[first]
    if source == "table":
        k = np.asarray(links).shape[1]
        table = np.where(link_keep, node_map[np.clip(ends[:, 1], 0, max(n - 1, 0))] if n else -1, -1).astype(np.int32).reshape(n, k)
        links_out, link_source = table[node_keep], None
    else:
        links_out = node_map[ends[link_keep]].astype(np.int32).reshape(-1, W)
        link_source = np.flatnonzero(link_keep).astype(np.int32)
    info = dict(components=K, kept=int(keep.sum()), nodes=int(node_keep.sum()), links=int(link_keep.sum()), bad_nodes=int((~good).sum()),
                bad_links=bad_links, isolated=int((good & ~touched).sum()), unsettled=0)
    return SimpleNamespace(labels=labels, n_nodes=n_nodes, n_links=n_links, box=box, extent=extent, keep=keep.astype(np.uint8), nodes=nodes,
                           node_map=node_map, links=links_out, link_source=link_source, labels_out=labels_out.astype(np.int32), info=info)
