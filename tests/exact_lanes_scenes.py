"""Scenes for the per-ray exact episode (MfmaSpec::exact_lanes), host half of
tests/test_gpu_exact_lanes.py; tests/test_exact_lanes_model.py asserts on the
CPU oracle what they are built to give.  Index-coded lights as in
closest_hit_scenes.py.

The images are rendered without pixel jitter (pixelRight = pixelUp = 0): the
ray of pixel (tx, ty) goes through the normalised viewport point ((2 tx - W) /
W, (2 ty - H) / H), so a triangle whose vertices lie on chosen viewport rays
is hit by exactly the pixels chosen, at any depth."""
import numpy as np

import closest_hit_scenes as S


def still_uniforms(width, height, n):
    """coded_uniforms without pixel jitter and defocus: one fixed ray per pixel."""
    u = S.coded_uniforms(width, height, n)
    for v in (u.pixelRight, u.pixelUp, u.defocusDiskRight, u.defocusDiskUp):
        v.x = v.y = v.z = 0.0
    return u


def _v3(v):
    return np.array([v.x, v.y, v.z], dtype=np.float64)


def _point(u, xn, yn, depth):
    """The point at `depth` viewport distances along the ray through (xn, yn)."""
    return _v3(u.cameraPos) + depth * (_v3(u.viewportFront) + xn * _v3(u.viewportRight) + yn * _v3(u.viewportUp))


def _facing(u, tri):
    """tri (3 points) wound so that its normal (b - a) x (c - a) looks at the camera."""
    a, b, c = tri
    n = np.cross(b - a, c - a)
    return (a, b, c) if np.dot(n, _v3(u.cameraPos) - a) > 0 else (a, c, b)


def _pack(u, tris):
    a, b, c = (np.array([_facing(u, t)[k] for t in tris], dtype=np.float32) for k in range(3))
    return S._triangles(a, b, c)


def _norm(width, height, px, py):
    return (2 * px - width) / width, (2 * py - height) / height


def _pixel_triangle(u, width, height, px, py, depth, size=0.4):
    """A small triangle around pixel (px, py)'s ray only (size in pixels, < 0.5)."""
    xn, yn = _norm(width, height, px, py)
    dx, dy = 2 * size / width, 2 * size / height
    return [_point(u, xn - dx, yn - dy, depth), _point(u, xn + dx, yn - dy, depth), _point(u, xn, yn + dy, depth)]


def one_ray_each(width, height):
    """width x height triangles (<= 64: one wave), triangle i hit by pixel i's
    ray alone (i = ty * width + tx in a scrambled order, so that a triangle's
    index says nothing about its ray's lane): every ray's mask is one bit."""
    n = width * height
    u = still_uniforms(width, height, n)
    order = (np.arange(n) * 7 + 3) % n if np.gcd(7, n) == 1 else (np.arange(n) * 5 + 3) % n
    assert len(set(order.tolist())) == n
    tris = [None] * n
    for p in range(n):
        tris[int(order[p])] = _pixel_triangle(u, width, height, p % width, p // width, 1.0 + 0.01 * (p % 5))
    return _pack(u, tris), S.code_materials(n), u, order


def one_ray_many(width, height, n, px, py):
    """n triangles stacked on pixel (px, py)'s ray (nearest = the highest
    index: the bound improves at every test); the other rays hit nothing."""
    u = still_uniforms(width, height, n)
    tris = [_pixel_triangle(u, width, height, px, py, 2.0 - i / n) for i in range(n)]
    return _pack(u, tris), S.code_materials(n), u


def all_rays_but_one(width, height, n):
    """n large triangles that cover every pixel but (0, 0) (the edge px + py =
    1/2 passes between it and its neighbours), nearest = the highest index."""
    u = still_uniforms(width, height, n)
    tris = []
    for i in range(n):
        depth = 2.0 - i / n
        corners = [(0.5 + 60.0, -60.0), (120.0, 120.0), (0.5 - 60.0, 60.0)]
        tris.append([_point(u, *_norm(width, height, px, py), depth) for px, py in corners])
    return _pack(u, tris), S.code_materials(n), u


def plane_fan(n, families):
    """S.fan (every triangle covers every pixel: slot k of the sweep's hot list
    is triangle k) with, for each family (lower, upper) and its plane (a, c):
    both indices replaced by the same triangle on z = a x + c, in front of the
    fan's planes, so that every family is the closest hit somewhere and ties
    exactly with itself."""
    t = S.fan(n, S.FAN_SEED, "shuffled").copy()
    for (lo, hi), (a, c) in families:
        for k, (x, y) in zip("abc", ((-40.0, -20.0), (40.0, -20.0), (0.0, 50.0))):
            for i in (lo, hi):
                t[k][i, :3] = (x, y, np.float32(a * x + c))
    return t, S.code_materials(n)


# the tie families: slots 31 | 32 (two rounds), bits 15 | 16 (the two halves of a ray's mask, which the
# block swap joins), and two groups (40 in group 1, 70 in group 2); each wins a stripe of the image
TIE_N = 72
TIE_FAMILIES = (((31, 32), (0.5, 1.0)), ((15, 16), (-0.5, 1.0)), ((40, 70), (0.0, 1.25)))
