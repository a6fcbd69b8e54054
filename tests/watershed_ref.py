"""
Yardstick of the watershed split, written from the definition in include/ddpm3d.h and not from the
kernels: numpy on the host, neighbours by shifted slices, every reduction sequential.  Also the case generators of the
two test tiers.
"""

import itertools

import numpy as np


def offsets(connectivity, forward=False):
    """the neighbour offsets (dz, dy, dx) of a connectivity; forward: those that follow a voxel in raster order"""
    order = {6: 1, 18: 2, 26: 3}[connectivity]
    out = []
    for o in itertools.product((-1, 0, 1), repeat=3):
        nz = sum(c != 0 for c in o)
        if 1 <= nz <= order and (not forward or o > (0, 0, 0)):
            out.append(o)
    return out


def foreground(height, labels):
    height = np.asarray(height)
    return (np.asarray(labels) > 0) & (height == height)


def _shifted(shape, o):
    """slices (of a voxel, of its neighbour at offset o) over all voxels whose neighbour lies in the volume"""
    here, there = [], []
    for n, d in zip(shape, o):
        here.append(slice(max(0, -d), n - max(0, d)))
        there.append(slice(max(0, d), n - max(0, -d)))
    return tuple(here), tuple(there)


def neighbour_pairs(height, labels, connectivity, forward):
    """yields (flat index of v, flat index of its neighbour u) arrays, one pair of arrays per offset (step 2)"""
    height, labels = np.asarray(height), np.asarray(labels)
    fg = foreground(height, labels)
    index = np.arange(height.size, dtype=np.int64).reshape(height.shape)
    for o in offsets(connectivity, forward):
        here, there = _shifted(height.shape, o)
        ok = fg[here] & fg[there] & (labels[here] == labels[there])
        yield index[here][ok], index[there][ok]


def parents(height, labels, connectivity):
    """step 4: the flat index of the voxel of greatest key among each voxel and its neighbours; -1 on background"""
    height = np.asarray(height, dtype=np.float32)
    h = height.reshape(-1)
    fg = foreground(height, labels).reshape(-1)
    best = np.where(fg, np.arange(h.size, dtype=np.int64), -1)
    for v, u in neighbour_pairs(height, labels, connectivity, forward=False):
        b = best[v]
        wins = (h[u] > h[b]) | ((h[u] == h[b]) & (u < b))
        best[v[wins]] = u[wins]
    return best


def basins(height, labels, connectivity):
    """-> (peaks int32 of height's shape, the number of peaks, the longest parent chain in links)"""
    p = parents(height, labels, connectivity)
    fg = p >= 0
    at = np.where(fg, np.arange(p.size, dtype=np.int64), -1)
    longest = 0
    while True:                                           # one link per round: the rounds are the longest chain
        nxt = np.where(fg, p[np.maximum(at, 0)], -1)
        if np.array_equal(nxt, at):
            break
        at = nxt
        longest += 1
    n = int((at == np.arange(at.size)).sum())
    return at.astype(np.int32).reshape(np.shape(height)), n, longest


def saddles(height, labels, peaks, connectivity):
    """step 5 -> (pairs (E, 2) int32 ascending, saddle (E,) float32)"""
    h = np.asarray(height, dtype=np.float32).reshape(-1)
    pk = np.asarray(peaks).reshape(-1).astype(np.int64)
    best = {}
    for v, u in neighbour_pairs(height, labels, connectivity, forward=True):
        differ = pk[v] != pk[u]
        v, u = v[differ], u[differ]
        a, b = np.minimum(pk[v], pk[u]), np.maximum(pk[v], pk[u])
        s = np.minimum(h[v], h[u])
        for ai, bi, si in zip(a.tolist(), b.tolist(), s.tolist()):
            k = (ai, bi)
            if k not in best or si > best[k]:
                best[k] = si
    keys = sorted(best)
    pairs = np.array(keys, dtype=np.int32).reshape(-1, 2)
    return pairs, np.array([best[k] for k in keys], dtype=np.float32)


def key_greater(h, i, j):
    """key(i) > key(j) for voxels i != j of heights h[i], h[j]"""
    return h[i] > h[j] or (h[i] == h[j] and i < j)


def merge(height, pairs, saddle, prominence):
    """step 6 on peaks given by their flat indices -> {peak: the peak of its cluster}"""
    h = {int(p): float(np.asarray(height, dtype=np.float32).reshape(-1)[p]) for p in np.unique(pairs)}
    edges = sorted((-float(s), int(a), int(b), float(s)) for (a, b), s in zip(pairs, saddle))
    cluster = {p: p for p in h}                           # peak -> its cluster's peak, kept flat

    for _, a, b, s in edges:
        ca, cb = cluster[a], cluster[b]
        if ca == cb:
            continue
        hi, lo = (ca, cb) if key_greater(h, ca, cb) else (cb, ca)
        with np.errstate(invalid="ignore"):
            stands = bool(np.float64(h[lo]) - np.float64(s) >= np.float64(prominence))
        if not stands:
            for p in cluster:
                if cluster[p] == lo:
                    cluster[p] = hi
    return cluster


def number(piece_of_voxel):
    """step 7: any per-voxel piece id (-1 = background) -> (labels 1..n in raster order of first voxels, n)"""
    flat = np.asarray(piece_of_voxel).reshape(-1)
    out = np.zeros(flat.size, dtype=np.int32)
    seen = {}
    for i in np.flatnonzero(flat >= 0).tolist():
        out[i] = seen.setdefault(int(flat[i]), len(seen) + 1)
    return out.reshape(np.shape(piece_of_voxel)), len(seen)


def split(labels, height, prominence, connectivity=26):
    """steps 1-7 -> (labels', n', info as metrics.split_components)"""
    labels = np.asarray(labels)
    peaks, n_basins, _ = basins(height, labels, connectivity)
    pairs, saddle = saddles(height, labels, peaks, connectivity)
    cluster = merge(height, pairs, saddle, prominence)
    flat = peaks.reshape(-1).astype(np.int64)
    piece = np.array([cluster.get(int(p), int(p)) if p >= 0 else -1 for p in flat.tolist()], dtype=np.int64)
    out, n = number(piece.reshape(labels.shape))
    parent = [0] * n
    for new, old in zip(out.reshape(-1).tolist(), labels.reshape(-1).tolist()):
        if new:
            parent[new - 1] = old
    info = {"n_before": int(labels.max()) if labels.size else 0, "n_basins": n_basins, "n_edges": int(pairs.shape[0]),
            "n_after": n, "parent": parent}
    return out, n, info


# ------------------------------------------------------------------------------------------------ cases
def two_blobs(noise=0.0, seed=0, shape=(12, 20, 28)):
    """(height, labels): two overlapping Gaussian blobs, peaks 1.0 and 0.8, sigma 3.5, centres 10 apart along W; one
    component at threshold 0.3"""
    z, y, x = np.indices(shape).astype(np.float64)
    c = (shape[0] // 2, shape[1] // 2)

    def g(x0, a):
        return a * np.exp(-((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - x0) ** 2) / (2 * 3.5 ** 2))

    clean = g(shape[2] // 2 - 5, 1.0) + g(shape[2] // 2 + 5, 0.8)
    h = clean + noise * np.random.default_rng(seed).standard_normal(shape) if noise else clean
    return h.astype(np.float32), (clean > 0.3).astype(np.int32)


def random_case(shape, seed, quantise=False, specials=True):
    """(height, labels): random fp32 heights, a random volume of blocks of 5 labels (0 among them) so that voxels of
    different labels touch; NaN and both infinities sprinkled in; quantise: 4 levels only, for ties"""
    rng = np.random.default_rng(seed)
    block = [max(1, (n + 2) // 3) for n in shape]
    coarse = rng.integers(0, 5, size=[-(-n // b) for n, b in zip(shape, block)])
    labels = coarse
    for axis, b in enumerate(block):
        labels = np.repeat(labels, b, axis=axis)
    labels = labels[:shape[0], :shape[1], :shape[2]].astype(np.int32)
    h = rng.standard_normal(shape).astype(np.float32)
    if quantise:
        h = np.floor(rng.random(shape) * 4).astype(np.float32)
    if specials:
        r = rng.random(shape)
        h[r < 0.03] = np.nan
        h[(r >= 0.03) & (r < 0.06)] = np.inf
        h[(r >= 0.06) & (r < 0.09)] = -np.inf
    return h, np.ascontiguousarray(labels)


def ramp(n=300, rising=True):
    h = np.arange(n, dtype=np.float32).reshape(1, 1, n)
    return (h if rising else h[:, :, ::-1].copy()), np.ones((1, 1, n), dtype=np.int32)


def serpentine(shape=(9, 9, 70)):
    """(height, labels, path length): a 6-connected path that takes every other row of every other plane, its voxels
    numbered along it; no two voxels of the path touch by a face unless they follow each other"""
    D, H, W = shape
    path = []
    right = True
    for zi, z in enumerate(range(0, D, 2)):
        rows = list(range(0, H, 2))
        if zi % 2:
            rows.reverse()
        for yi, y in enumerate(rows):
            xs = list(range(W)) if right else list(range(W - 1, -1, -1))
            path += [(z, y, x) for x in xs]
            right = not right
            if yi + 1 < len(rows):
                path.append((z, (y + rows[yi + 1]) // 2, xs[-1]))
        if z + 2 < D:
            path.append((z + 1, rows[-1], path[-1][2]))
    h = np.zeros(shape, dtype=np.float32)
    lab = np.zeros(shape, dtype=np.int32)
    for i, p in enumerate(path):
        h[p] = i
        lab[p] = 1
    return h, lab, len(path)


def constant_box(shape=(9, 17, 130)):
    return np.full(shape, 2.5, dtype=np.float32), np.ones(shape, dtype=np.int32)


def u_plateau(shape=(3, 9, 70)):
    """a constant U: two arms along H joined at the high-H end; the arm that does not hold the lowest index has a
    lowest voxel of its own whose neighbours all have larger indices"""
    lab = np.zeros(shape, dtype=np.int32)
    lab[:, :, 2:5] = 1
    lab[:, :, 40:43] = 1
    lab[:, shape[1] - 2:, 2:43] = 1
    return np.where(lab > 0, 1.0, 0.0).astype(np.float32), lab


def two_balls(shape=(13, 16, 30), r=5.5, gap=7):
    """a uint8 mask of two overlapping balls, centres `gap` apart along W: one component with a waist"""
    z, y, x = np.indices(shape)
    c = (shape[0] // 2, shape[1] // 2, shape[2] // 2)
    m = np.zeros(shape, dtype=bool)
    for x0 in (c[2] - gap // 2 - 1, c[2] + (gap + 1) // 2 - 1):
        m |= (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - x0) ** 2 <= r * r
    return m.astype(np.uint8)


def random_graph(n, edges, seed, levels=None):
    """(peak_index ascending, peak_height, pairs (E, 2) unique ascending, saddle) with saddle <= both peaks' heights;
    levels: heights and saddles from that many values only (ties)"""
    rng = np.random.default_rng(seed)
    index = np.sort(rng.choice(10 * n, size=n, replace=False)).astype(np.int64)
    draw = (lambda k: rng.integers(0, levels, size=k).astype(np.float32)) if levels else \
        (lambda k: rng.random(k).astype(np.float32))
    height = draw(n) + (levels or 1)
    a = rng.integers(0, n, size=edges)
    b = rng.integers(0, n, size=edges)
    keep = a != b
    lo, hi = np.minimum(a, b)[keep], np.maximum(a, b)[keep]
    uniq = np.unique(np.stack([lo, hi], axis=1), axis=0)
    pairs = index[uniq]
    saddle = np.minimum(np.minimum(height[uniq[:, 0]], height[uniq[:, 1]]), draw(len(uniq)) + (levels or 1) / 2.0)
    return index, height.astype(np.float32), pairs, saddle.astype(np.float32)
