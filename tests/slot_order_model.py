"""The CPU model behind DESIGN.md "Slot order": model rays of config B, the
instruction prices of the resident kernel's group loop, the cost of a cluster
table on those rays and the best contiguous table for them.

Rays: N_PIXELS random pixels of the bench view, 64 jittered rays each; the
closest hits by the oracle; every bounce a cosine scatter about the hit's
normal, SEGMENTS segments in all.  One (pixel, segment) is one wave's sweep;
a ray that left the scene is a dead lane from then on.
"""
import numpy as np

import oracle
import rt2

N_PIXELS, SEGMENTS, SEED = 500, 9, 20261020
PER_SWEEP = 38.0
_cache = {}


def price32(n):
    return 28.0 + 53.0 * (n // 2) + 27.0 * (n % 2)


def price16(n):
    return min(38.0 + 31.0 * (n // 2) + 16.0 * (n % 2), price32(n))


def cluster_price(n, c, compact):
    """Vector instructions of one cluster of n groups in one sweep; c = the live rays that need it (array)."""
    c = np.asarray(c)
    if not compact:
        return np.full(c.shape, 8.0 + 51.5 * n)
    body = np.where(c == 0, 0.0, np.where(c <= 16, price16(n), np.where(c <= 32, price32(n), 51.5 * n)))
    return 27.0 + 4.0 + body


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def model_rays(seed=SEED, pixels=N_PIXELS, segments=SEGMENTS):
    """-> list of (o [64 w, 3], d, live [w, 64]) per segment, of config B's scene (cached)."""
    key = (seed, pixels, segments)
    if key in _cache:
        return _cache[key]
    sd, spec = rt2.build_config_scene("B")
    tris = sd.triangles()
    u = rt2.offline_uniforms(spec.width, spec.height, spec.bounces, spec.rays, sd.num_triangles)
    rng = np.random.default_rng(seed)
    v3 = lambda v: np.array([v.x, v.y, v.z], np.float64)
    cam, right, up, front = v3(u.cameraPos), v3(u.viewportRight), v3(u.viewportUp), v3(u.viewportFront)
    W, H = int(u.width), int(u.height)
    px = np.repeat(rng.integers(0, W, pixels), 64) + rng.random(64 * pixels)
    py = np.repeat(rng.integers(0, H, pixels), 64) + rng.random(64 * pixels)
    end = front[None] + right[None] * ((2 * px - W) / W)[:, None] + up[None] * ((2 * py - H) / H)[:, None]
    o = np.broadcast_to(cam, end.shape).astype(np.float32)
    d = _unit(end).astype(np.float32)
    live = np.ones(64 * pixels, bool)
    a, b, c = (tris[k][:, :3].astype(np.float64) for k in "abc")
    nrm = _unit(np.cross(b - a, c - a) + 1e-300)
    out = []
    for _ in range(segments):
        out.append((o.copy(), d.copy(), live.reshape(pixels, 64).copy()))
        dst, idx, _, _ = oracle.closest_hits(tris, o, d)
        hit = live & (idx >= 0)
        n = nrm[np.maximum(idx, 0)]
        n = np.where((np.sum(n * d, -1) > 0)[:, None], -n, n)
        s = _unit(rng.normal(size=(len(o), 3)))
        nd = _unit(n + s * 0.999)
        no = o.astype(np.float64) + d.astype(np.float64) * dst[:, None].astype(np.float64) + n * 1e-4
        o = np.where(hit[:, None], no, o).astype(np.float32)
        d = np.where(hit[:, None], nd, d).astype(np.float32)
        live = hit
    _cache[key] = (tris, out)
    return _cache[key]


def kill_lanes(rays, frac, seed=1):
    """The same rays with a further share `frac` of the lanes dead."""
    rng = np.random.default_rng(seed)
    return [(o, d, live & (rng.random(live.shape) >= frac)) for o, d, live in rays]


def need_counts(table, rays):
    """[sweeps, n clusters]: the live rays of every sweep that need each cluster of `table` (rt2_cluster_need)."""
    n = int(table["n"])
    cols = []
    for o, d, live in rays:
        bits = rt2.cluster_need(table, o, d).reshape(live.shape)
        cols.append(np.stack([((bits >> k & 1).astype(bool) & live).sum(1) for k in range(n)], 1))
    return np.concatenate(cols, 0)


def table_cost(table, rays):
    """Mean vector instructions of the group loop per sweep under `table` (n = 0: the loop without clusters)."""
    n = int(table["n"])
    if n == 0:
        raise ValueError("a table without clusters has no ranges to price")
    cnt = need_counts(table, rays)
    tot = np.full(len(cnt), PER_SWEEP)
    for k, c in enumerate(table["c"][:n]):
        g0, g1 = int(c["g0"]), int(c["g1_flags"]) & 0xffff
        tot = tot + cluster_price(g1 - g0, cnt[:, k], bool(int(c["g1_flags"]) & rt2.CLUSTER_COMPACT))
    return float(tot.mean())


_need_cache = {}


def range_need(tris, rays_key, rays, like):
    """(i, j) -> packed need bits [sweeps, 8] uint8 of the compact cluster of groups [i, j) of tris, its box padded
    like the table `like`'s (cached per triangle array and ray set: the bits do not depend on which lanes live)."""
    key = (tris.tobytes(), rays_key)
    if key in _need_cache:
        return _need_cache[key]
    ng = (len(tris) + 31) // 32
    v = np.stack([tris["a"][:, :3], tris["b"][:, :3], tris["c"][:, :3]], 1).astype(np.float64)
    glo = np.stack([v[32 * g:32 * g + 32].min((0, 1)) for g in range(ng)])
    ghi = np.stack([v[32 * g:32 * g + 32].max((0, 1)) for g in range(ng)])
    all_ranges = [(i, j) for i in range(ng) for j in range(i + 1, ng + 1)]
    out = {}
    K = rt2.MAX_CLUSTERS
    for s0 in range(0, len(all_ranges), K):
        part = all_ranges[s0:s0 + K]
        t = np.zeros(1, dtype=rt2.CLUSTER_TABLE_DTYPE)[0]
        t["far_o"], t["pad_abs"], t["n"] = like["far_o"], like["pad_abs"], len(part)
        for k, (i, j) in enumerate(part):  # rt2_cluster_need reads the boxes, not the ranges
            t["c"][k]["g0"], t["c"][k]["g1_flags"] = i, j | rt2.CLUSTER_COMPACT
            t["c"][k]["lo"] = glo[i:j].min(0).astype(np.float32) - like["pad_abs"]
            t["c"][k]["hi"] = ghi[i:j].max(0).astype(np.float32) + like["pad_abs"]
        bits = np.concatenate([rt2.cluster_need(t, o, d).reshape(live.shape) for o, d, live in rays], 0)
        for k, r in enumerate(part):
            out[r] = np.packbits((bits >> k & 1).astype(bool), axis=1)
    _need_cache[key] = out
    return out


_POP8 = np.array([bin(x).count("1") for x in range(256)], np.int64)


def best_contiguous_table(tris, rays, like, rays_key=SEED):
    """The cheapest table of contiguous ranges over tris' groups for these rays, every price known: a dynamic
    programme over (clusters, end group).  like: a table whose padding the boxes take.  rays_key names the rays
    whatever lanes live.  -> (ranges, cost)."""
    ng = (len(tris) + 31) // 32
    need = range_need(tris, rays_key, rays, like)
    live = np.packbits(np.concatenate([l for _, _, l in rays], 0), axis=1)
    price = {}
    for (i, j), bits in need.items():
        c = _POP8[bits & live].sum(1)
        comp = float(cluster_price(j - i, c, True).mean())
        full = 8.0 + 51.5 * (j - i)
        price[i, j] = (comp, True) if comp < full else (full, False)
    K = rt2.MAX_CLUSTERS
    inf = float("inf")
    cost = [[inf] * (ng + 1) for _ in range(K + 1)]
    frm = [[None] * (ng + 1) for _ in range(K + 1)]
    cost[0][0] = 0.0
    for k in range(1, K + 1):
        for j in range(1, ng + 1):
            for i in range(j):
                v = cost[k - 1][i] + price[i, j][0]
                if v < cost[k][j]:
                    cost[k][j], frm[k][j] = v, i
    bk = min(range(1, K + 1), key=lambda k: cost[k][ng])
    ranges, j = [], ng
    for k in range(bk, 0, -1):
        i = frm[k][j]
        ranges.append((i, j, price[i, j][1]))
        j = i
    return ranges[::-1], PER_SWEEP + cost[bk][ng]
