"""Test-only scene builders for the rasterizer's tie tests (tests/test_gpu_raster_ties.py and the host tests of
tests/test_raster_oracle.py): meshes whose vertices, edges and depths fall exactly on, or within rounding of, the
pixel-centre lattice, where the coverage test's tie rule, canonical edge order and depth-tie rule decide.  numpy / torch
on the CPU only.  Pixel units: pixel (px, py) has its corners at (px, py) .. (px + 1, py + 1) and its centre at
(px + 1/2, py + 1/2); a point c (pixel units) of an image N pixels wide has NDC 2 c / N - 1.

Every builder returns pos (V,4) float32 clip space and tri (T,3) int32 (plus what its docstring says)."""
import numpy as np
import torch


def _ndc(c, N):
    return 2.0 * np.asarray(c, dtype=np.float64) / N - 1.0


def _clip(X, Y, w, z=0.0):
    """float32 clip positions (X w, Y w, z w, w): NDC rounded to float32 first, then one float32 product each"""
    X, Y, w = (np.asarray(a, dtype=np.float64).astype(np.float32) for a in (X, Y, w))
    z = np.broadcast_to(np.asarray(z, dtype=np.float32), w.shape)
    return torch.from_numpy(np.stack([X * w, Y * w, z * w, w], -1).astype(np.float32))


def _shuffle(pos, tri, seed):
    """renumber the vertices (which changes every edge's canonical endpoint order), rotate and flip every triple"""
    rng = np.random.default_rng(seed)
    V = pos.shape[0]
    perm = rng.permutation(V)  # old vertex i becomes perm[i]
    new_pos = torch.empty_like(pos)
    new_pos[torch.from_numpy(perm)] = pos
    t = perm[np.asarray(tri, dtype=np.int64)]
    rot = rng.integers(0, 3, len(t))
    t = np.stack([t[np.arange(len(t)), (rot + j) % 3] for j in range(3)], 1)
    flip = rng.integers(0, 2, len(t)).astype(bool)
    t[flip] = t[flip][:, [0, 2, 1]]
    return new_pos, torch.from_numpy(t.astype(np.int32))


def _checker_tris(nx, ny):
    """two triangles per square of an (nx + 1) x (ny + 1) vertex grid (vertex (a, b) = b (nx + 1) + a), the diagonal
    alternating like a checkerboard"""
    tri = []
    vid = lambda a, b: b * (nx + 1) + a
    for b in range(ny):
        for a in range(nx):
            v00, v10, v11, v01 = vid(a, b), vid(a + 1, b), vid(a + 1, b + 1), vid(a, b + 1)
            if (a + b) % 2 == 0:
                tri += [(v00, v10, v11), (v00, v11, v01)]
            else:
                tri += [(v00, v10, v01), (v10, v11, v01)]
    return np.asarray(tri, dtype=np.int64)


def lattice_grid(H, W, k, w_mode, seed):
    """The whole image tiled by k x k pixel squares with vertices at pixel corners, each square split by a diagonal
    that alternates like a checkerboard: every diagonal runs through pixel centres.  w_mode: "one", "pow2" (w in
    {1/2, 1, 2}) or "rand" (uniform in [0.5, 2): x = fl(X w) is then inexact and the centres are near-ties)."""
    assert H % k == 0 and W % k == 0
    rng = np.random.default_rng(1000 + seed)
    nx, ny = W // k, H // k
    a, b = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="xy")
    a, b = a.reshape(-1), b.reshape(-1)
    n = a.size
    if w_mode == "one":
        w = np.ones(n)
    elif w_mode == "pow2":
        w = rng.choice([0.5, 1.0, 2.0], n)
    elif w_mode == "rand":
        w = rng.uniform(0.5, 2.0, n)
    else:
        raise ValueError(w_mode)
    pos = _clip(_ndc(a * k, W), _ndc(b * k, H), w)
    return _shuffle(pos, _checker_tris(nx, ny), seed)


def centre_grid(N, k):
    """Vertices at the pixel centres k, 2k, .., N - k of an N x N image (N a power of two: every coordinate dyadic),
    w = 1, checkerboard diagonals, alternating windings: every vertex and every edge (horizontal, vertical, diagonal)
    passes exactly through pixel centres.  The mesh covers the rectangle between the centres of pixels k and N - k."""
    assert N & (N - 1) == 0 and N % k == 0 and N // k >= 3
    m = N // k - 2  # squares per side
    a, b = np.meshgrid(np.arange(m + 1), np.arange(m + 1), indexing="xy")
    a, b = a.reshape(-1), b.reshape(-1)
    pos = _clip(_ndc((a + 1) * k + 0.5, N), _ndc((b + 1) * k + 0.5, N), np.ones(a.size))
    tri = _checker_tris(m, m)
    tri[1::2] = tri[1::2][:, [0, 2, 1]]
    return pos, torch.from_numpy(tri.astype(np.int32))


def fan(N, n):
    """n triangles around a hub at the centre of pixel (N/2, N/2); the rim vertices at pixel corners, evenly spaced
    along the square ring 2 .. N - 2 (N a power of two, w = 1: exact).  All n triangles tie at the hub."""
    assert N & (N - 1) == 0 and N >= 8
    lo, hi = 2, N - 2
    side = hi - lo
    ring = [(lo + i, lo) for i in range(side)] + [(hi, lo + i) for i in range(side)] + \
           [(hi - i, hi) for i in range(side)] + [(lo, hi - i) for i in range(side)]
    rim = [ring[(i * len(ring)) // n] for i in range(n)]
    assert len(set(rim)) == n
    pts = np.asarray([(N // 2 + 0.5, N // 2 + 0.5)] + rim, dtype=np.float64)
    pos = _clip(_ndc(pts[:, 0], N), _ndc(pts[:, 1], N), np.ones(len(pts)))
    tri = np.asarray([(0, 1 + i, 1 + (i + 1) % n) for i in range(n)], dtype=np.int32)
    return pos, torch.from_numpy(tri)


def mixed_edge(W, d, seed):
    """Two triangles of a W x W image sharing the edge from the pixel corner A to A + n d, d = (odd, odd), so that the
    edge passes through the pixel centres A + (m + 1/2) d.  Its endpoints carry random non-dyadic w > 0.  Triangle
    `first` has its third vertex in front of the camera (every w > 0); the other one's third vertex has w < 0 and
    projects onto the first one's side of the edge, so its visible part lies on the other side.  Vertex numbers and
    windings are shuffled.  Returns pos (4,4), tri (2,3) and the on-edge pixels (P,2) int64 = (px, py) that are more
    than one pixel from both endpoints."""
    dx, dy = d
    assert dx % 2 == 1 and dy % 2 == 1 and dx > 0 and dy > 0
    rng = np.random.default_rng(7000 + seed)
    n = (W - 8) // max(dx, dy)
    A = np.array([rng.integers(2, W - 2 - n * dx + 1), rng.integers(2, W - 2 - n * dy + 1)], dtype=np.float64)
    B = A + n * np.array([dx, dy], dtype=np.float64)
    side = 1.0 if rng.integers(0, 2) else -1.0
    perp = side * np.array([-dy, dx], dtype=np.float64) / np.hypot(dx, dy)
    mid = 0.5 * (A + B)
    P1 = np.round(mid + perp * (0.3 * W) + rng.uniform(-2, 2, 2))         # in front, a pixel corner
    Q = np.round(mid + perp * (0.45 * W) + rng.uniform(-3, 3, 2)) + 0.25  # projection of the vertex behind the camera
    pts = np.stack([A, B, P1, Q])
    w = rng.uniform(0.5, 2.0, 4)
    w[3] = -w[3]
    pos = _clip(_ndc(pts[:, 0], W), _ndc(pts[:, 1], W), w)
    pos, tri = _shuffle(pos, np.array([[0, 1, 2], [1, 0, 3]]), 31 * seed + W + dx)
    m = np.arange(n) + 0.5
    c = A[None] + m[:, None] * np.array([dx, dy], dtype=np.float64)  # pixel centres: half-integers
    keep = (np.hypot(*(c - A).T) > 1.0) & (np.hypot(*(c - B).T) > 1.0)
    pix = np.floor(c[keep]).astype(np.int64)
    assert (pix >= 0).all() and (pix < W).all() and len(pix) > 0
    return pos, tri, torch.from_numpy(pix)


def coincident_quads(N, signed_zero=False):
    """Two quads with the same corners (pixel corners 2 and N - 2 of an N x N image, N a power of two; separate
    vertex entries, w = 1) at the same depth: z = 0.25 for both, or, with signed_zero, z = +0.0 for the first quad
    and z = -0.0 for the second.  Triangles 0, 1 are the first quad, 2, 3 the second."""
    assert N & (N - 1) == 0 and N >= 8
    c = _ndc(np.array([2, N - 2, N - 2, 2]), N), _ndc(np.array([2, 2, N - 2, N - 2]), N)
    X, Y = np.tile(c[0], 2), np.tile(c[1], 2)
    z = np.array([0.0] * 4 + [-0.0] * 4, dtype=np.float32) if signed_zero else np.full(8, 0.25, dtype=np.float32)
    pos = _clip(X, Y, np.ones(8))
    pos[:, 2] = torch.from_numpy(z)
    tri = torch.tensor([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], dtype=torch.int32)
    return pos, tri


def square(N, on_centres):
    """An axis-aligned square of two triangles, w = 1, in an N x N image (N a power of two): corners on the pixel
    centres 3 and N - 4 (vertices exactly on scanlines) or on the pixel corners 3 and N - 3 (the silhouette crosses
    every pair exactly half way, s = 0.5)."""
    lo, hi = (3.5, N - 3.5) if on_centres else (3.0, N - 3.0)
    X, Y = _ndc(np.array([lo, hi, hi, lo]), N), _ndc(np.array([lo, lo, hi, hi]), N)
    return _clip(X, Y, np.ones(4)), torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)


def split_quad(flip):
    """the full-screen quad [-1, 1]^2 split along its diagonal (through the pixel centres of a square image), in
    either winding"""
    pos = torch.tensor([[-1.0, -1, 0, 1], [1, -1, 0, 1], [1, 1, 0, 1], [-1, 1, 0, 1]])
    tri = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    return pos, (tri[:, [0, 2, 1]].contiguous() if flip else tri)
