"""Test-only numpy oracle of the mesh contract (include/tt_abi.h, "mesh regularisers and outlier removal"; DESIGN.md
section 13): edges, face components with a union-find of its own, outlier compaction, and both regularisers with their
gradients in float64.  tests/golden/reference_mesh_ops.npz pins the edges and losses to the reference's own
threestudio/models/mesh.py; remove_outlier has no golden (trimesh is absent), so this file's reading of the contract
is its oracle.
"""
import numpy as np

COS_EPS = 1e-8  # torch.cosine_similarity's default eps


def face_edges(tri):
    """(3T,2) the face edges 3f + k = (tri[f,k], tri[f,(k+1)%3]), each row sorted"""
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    e = np.stack([tri, tri[:, [1, 2, 0]]], axis=-1).reshape(-1, 2)
    return np.sort(e, axis=1)


def edges(tri):
    """threestudio Mesh._compute_edges: unique sorted rows, lexicographic, self pairs included"""
    e = face_edges(tri)
    if len(e) == 0:
        return np.zeros((0, 2), dtype=np.int64)
    return np.unique(e, axis=0)


def neighbours(n_vert, tri):
    """per vertex the sorted list of its neighbours over the unique edges, self pairs dropped"""
    nb = [[] for _ in range(n_vert)]
    for a, b in edges(tri).tolist():
        if a != b:
            nb[a].append(b)
            nb[b].append(a)
    return [sorted(x) for x in nb]


def face_components(tri):
    """(T,) label per face = the smallest face index of its component; faces are joined by an edge that exactly two
    face edges use (an edge used once or by three or more face edges joins nothing)."""
    T = len(tri)
    parent = list(range(T))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    groups = {}
    for i, (a, b) in enumerate(face_edges(tri).tolist()):
        groups.setdefault((a, b), []).append(i // 3)
    for faces in groups.values():
        if len(faces) == 2:
            ra, rb = find(faces[0]), find(faces[1])
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(f) for f in range(T)], dtype=np.int64)


def remove_small_components(v_pos, tri, threshold):
    """Mesh.remove_outlier's contract: a float threshold t -> int(largest component's faces * t), an int as given;
    components with faces >= threshold stay; kept vertices (referenced by a kept face) and kept faces keep their
    original order; faces renumbered.  No faces: the mesh as it is."""
    v_pos = np.asarray(v_pos)
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    if len(tri) == 0:
        return v_pos, tri
    lab = face_components(tri)
    size = np.bincount(lab, minlength=len(tri))
    thr = int(size.max() * threshold) if isinstance(threshold, float) else threshold
    keep = size[lab] >= thr
    vkeep = np.zeros(len(v_pos), dtype=bool)
    vkeep[tri[keep].reshape(-1)] = True
    new_id = np.cumsum(vkeep) - 1
    return v_pos[vkeep], new_id[tri[keep]]


def laplacian(v_pos, tri):
    """(loss, d loss / d v_pos) in float64: loss = mean_i |sum_{j in N(i), j != i} (v_i - v_j)|"""
    v = np.asarray(v_pos, dtype=np.float64)
    V = len(v)
    nb = neighbours(V, tri)
    r = np.zeros_like(v)
    for i in range(V):
        if nb[i]:
            r[i] = len(nb[i]) * v[i] - v[nb[i]].sum(0)
    n = np.linalg.norm(r, axis=1)
    loss = n.mean() if V else float("nan")
    w = np.where(n[:, None] > 0, r / np.where(n > 0, n, 1.0)[:, None], 0.0) / max(V, 1)
    g = np.zeros_like(v)
    for k in range(V):
        if nb[k]:
            g[k] = len(nb[k]) * w[k] - w[nb[k]].sum(0)
    return float(loss), g


def vertex_normals(v_pos, tri):
    """Mesh._compute_vertex_normal in float64: area-weighted, (0,0,1) where |n|^2 <= 1e-20, normalised"""
    v = np.asarray(v_pos, dtype=np.float64)
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    fn = np.cross(v[tri[:, 1]] - v[tri[:, 0]], v[tri[:, 2]] - v[tri[:, 0]])
    n = np.zeros_like(v)
    for k in range(3):
        np.add.at(n, tri[:, k], fn)
    n = np.where((n * n).sum(1, keepdims=True) > 1e-20, n, np.array([0.0, 0.0, 1.0]))
    return n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-12)


def vertex_normals_torch(v_pos, tri):
    """vertex_normals in torch, in the dtype of v_pos and autograd-connected to it (the gradient arbiter of the mesh
    renderer's oracle); tests/test_mesh_renderer_oracle.py holds it to the numpy one"""
    import torch
    tri = torch.as_tensor(np.asarray(tri, dtype=np.int64).reshape(-1, 3))
    v0, v1, v2 = v_pos[tri[:, 0]], v_pos[tri[:, 1]], v_pos[tri[:, 2]]
    fn = torch.linalg.cross(v1 - v0, v2 - v0)
    n = torch.zeros_like(v_pos)
    for k in range(3):
        n = n.index_add(0, tri[:, k], fn)
    n = torch.where((n * n).sum(1, keepdim=True) > 1e-20, n, torch.tensor([0.0, 0.0, 1.0], dtype=n.dtype))
    return n / n.norm(dim=1, keepdim=True).clamp_min(1e-12)


def normal_consistency_of_normals(v_nrm, tri):
    """(loss, d loss / d v_nrm) in float64: mean over edges of 1 - cosine_similarity(n_a, n_b, eps=1e-8)"""
    x = np.asarray(v_nrm, dtype=np.float64)
    e = edges(tri)
    if len(e) == 0:
        return float("nan"), np.zeros_like(x)
    m = np.linalg.norm(x, axis=1)
    n = np.maximum(m, COS_EPS)
    xt = x / n[:, None]
    a, b = e[:, 0], e[:, 1]
    cos = (xt[a] * xt[b]).sum(1)
    xu = np.where(m[:, None] > 0, x / np.where(m > 0, m, 1.0)[:, None], 0.0)
    g = np.zeros_like(x)
    # d cos / d x_a = y_hat / n_a - cos / n_a * x_a / |x_a|, and symmetrically for b
    np.add.at(g, a, xt[b] / n[a, None] - (cos / n[a])[:, None] * xu[a])
    np.add.at(g, b, xt[a] / n[b, None] - (cos / n[b])[:, None] * xu[b])
    return float((1.0 - cos).mean()), -g / len(e)


def normal_consistency(v_pos, tri):
    """(loss, d loss / d v_pos) in float64, through the vertex normals (torch float64 autograd for that chain)"""
    import torch
    v = torch.tensor(np.asarray(v_pos, dtype=np.float64), requires_grad=True)
    t = torch.as_tensor(np.asarray(tri, dtype=np.int64).reshape(-1, 3))
    fn = torch.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]], dim=-1)
    n = torch.zeros_like(v)
    for k in range(3):
        n = n.index_add(0, t[:, k], fn)
    n = torch.where((n * n).sum(-1, keepdim=True) > 1e-20, n, torch.tensor([0.0, 0.0, 1.0], dtype=v.dtype))
    n = torch.nn.functional.normalize(n, dim=1)
    loss, g_n = normal_consistency_of_normals(n.detach().numpy(), tri)
    n.backward(torch.as_tensor(g_n))
    return loss, v.grad.numpy()


def hand_mesh():
    """v_pos (11,3) float32, tri (9,3) int64: a closed tetrahedron (faces 0-3) whose edge (1,2) is also used by
    face 4 (a non-manifold edge: it joins nothing), a strip of faces 4-5, a strip of faces 7-8, a degenerate face 6
    (6,6,7) whose repeated edge (6,7) is also used by face 7, and an unreferenced vertex 10.  Components by the
    contract: {0,1,2,3}, {4,5}, {6}, {7,8}."""
    rng = np.random.RandomState(7)
    v = rng.uniform(-1.0, 1.0, size=(11, 3)).astype(np.float32)
    tri = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2], [1, 2, 4], [2, 4, 5], [6, 6, 7], [6, 7, 8],
                    [7, 8, 9]], dtype=np.int64)
    return v, tri


def sheet(n):
    """v_pos (n*n, 3) float32 at z = 0, tri (2 (n-1)^2, 3) int64: an n x n vertex grid, vertex i * n + j at (i, j, 0);
    the cell with lowest corner a gives (a, a+n, a+1) and (a+1, a+n, a+n+1); all first faces, then all second faces"""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([i, j, np.zeros_like(i)], -1).reshape(-1, 3).astype(np.float32)
    a = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1).astype(np.int64)
    return v, np.concatenate([np.stack([a, a + n, a + 1], 1), np.stack([a + 1, a + n, a + n + 1], 1)])


def sphere_field(R, centre=(0.5, 0.5, 0.5), radius=0.3):
    x = np.linspace(0.0, 1.0, R)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    return (np.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) - radius).astype(np.float32)


def torus_field(R, big=0.28, small=0.1):
    x = np.linspace(0.0, 1.0, R) - 0.5
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    return (np.sqrt((np.sqrt(X ** 2 + Y ** 2) - big) ** 2 + Z ** 2) - small).astype(np.float32)


def blobs_field(R):
    """two spheres of different size plus three small blobs: five components of very different face counts"""
    parts = [sphere_field(R, (0.3, 0.3, 0.5), 0.2), sphere_field(R, (0.72, 0.7, 0.5), 0.14),
             sphere_field(R, (0.15, 0.85, 0.2), 0.045), sphere_field(R, (0.85, 0.15, 0.8), 0.05),
             sphere_field(R, (0.5, 0.85, 0.85), 0.06)]
    return np.minimum.reduce(parts)
