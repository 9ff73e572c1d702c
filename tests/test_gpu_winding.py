"""HIP winding number (tt_wind_*; ops.WindingTree, mesh_winding_number, mesh_contains, mesh_signed_distance;
Mesh.winding_number / contains / signed_distance; shape.MeshOBJ, ce_pq_loss, ShapeLoss) against the float64 restatement
tests/winding_reference.py.

The bar of every comparison of a winding number against float64 is BAR = 1.7e-5 absolute: an fp32 numpy restatement of
the same formula (fp32 pairs, double sum) measured on the cases of this file, points at least 1e-3 extents from the
surface, deviates from float64 by at most 9.1e-7 (sphere24), 6.4e-7 (torus32), 4.3e-6 (hand), 6.7e-7 (triangle),
1.1e-6 (two_clusters), 7.6e-7 (spanning); BAR is 4x the largest.  The points closer than that are at most 0.94 % of a
case (two_clusters; tests/test_winding_host.py checks the cap on the CPU).

The method error of the dipole tree (max |fast - exact| in float64 over the points away from the surface), which the
tests measure again from the restatement: sphere24 L=3 0.022 (beta 2) / 0.0085 (beta 3), L=1 0.0081 / 0.0013; torus32
L=3 0.032 / 0.013, L=1 0.017 / 0.0040; hand L=1 0.0023 / 0.00013; two_clusters L=1 0.0029 / 0.0010; spanning L=1
0.0024 / 0.00074; L=0 at most 0.0010 (triangle).  Points with a decision margin below 1e-4 are at most 3.4 % of a case
at these depths.  At the default depth of the two closed meshes (L=5: 0.022 / 0.0086 and 0.036 / 0.013) a point tests
some thousand nodes and 5-11 % of the points have one decision within 1e-4: test (d) keeps its 5 % cap and runs at L=1
and L=3; the default depth has a test of its own that asserts everything but that cap and prints the fraction.

The reference's own numbers cannot serve as golden vectors: igl is not installed where these tests were written, and
its fast winding number is an expansion of another order -- an approximation of the same exact sum, not of this tree."""
import os
import sys

import numpy as np
import pytest
import torch

from triplaneturbo_amd import ops, shape
from triplaneturbo_amd.isosurface import Mesh, kuhn_tet_grid

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distance_reference as D  # noqa: E402
import winding_reference as W  # noqa: E402

pytestmark = pytest.mark.gpu
BAR = 1.7e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def gpu(name, dev):
    v, t = W.mesh(name)
    return torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev)


def f64(x):
    return x.double().cpu().numpy()


# ---- a. exact against float64 ----
@pytest.mark.parametrize("name", W.MESHES)
def test_exact_matches_float64(dev, name):
    pts, w, away, _ = W.case(name)
    assert (~away).mean() <= 0.01
    bad = np.array([[0.1, np.nan, 0.2], [np.inf, 0.0, 0.0], [0.3, 0.1, -np.inf]], np.float32)
    allp = np.concatenate([pts[:700], bad[:1], pts[700:], bad[1:]])  # NaN in the middle of a wave, inf rows at the end
    tree = ops.WindingTree(*gpu(name, dev))
    got = ops.mesh_winding_number(torch.from_numpy(allp).to(dev), tree, exact=True)
    assert got.dtype == torch.float32 and got.shape == (len(allp),)
    rows = torch.tensor([700, len(allp) - 2, len(allp) - 1], device=dev)
    assert torch.isnan(got[rows]).all()
    keep = torch.ones(len(allp), dtype=torch.bool, device=dev)
    keep[rows] = False
    err = np.abs(f64(got[keep]) - w)
    print(f"{name}: N {len(pts)} T {tree.n_faces}  max |w - float64| = {err[away].max():.3e} away from the surface "
          f"({err[away].max() / BAR:.3f} of the bar), {err.max():.3e} over all points")
    assert np.isfinite(f64(got[keep])).all()
    assert (err[away] <= BAR).all()
    clean = ops.mesh_winding_number(torch.from_numpy(pts).to(dev), tree, exact=True)
    assert torch.equal(got[keep], clean)  # the other rows are unaffected, bit for bit
    # a mesh given as tensors builds its own root
    assert torch.equal(ops.mesh_winding_number(torch.from_numpy(pts).to(dev), *gpu(name, dev), exact=True), clean)


# ---- b. exact is bit-identical under launch shape and point order ----
@pytest.mark.parametrize("name", ["sphere24", "hand"])  # 1772 faces = 6 tiles of 256 + 236; 9 faces: below one tile
def test_exact_is_bit_identical_under_permutation_and_count(dev, name):
    pts = W.case(name)[0]
    tree = ops.WindingTree(*gpu(name, dev))
    assert tree.n_faces % 256 != 0
    p = torch.from_numpy(pts).to(dev)
    base = ops.mesh_winding_number(p, tree, exact=True)
    perm = torch.from_numpy(np.random.default_rng(22).permutation(len(pts))).to(dev)
    assert torch.equal(ops.mesh_winding_number(p[perm], tree, exact=True), base[perm])
    for n in (1, 63, 64, 65, 257, 1025):
        assert torch.equal(ops.mesh_winding_number(p[:n].contiguous(), tree, exact=True), base[:n])
        assert torch.equal(ops.mesh_winding_number(p[-n:].contiguous(), tree, exact=True), base[-n:])
    assert ops.mesh_winding_number(p[:0], tree, exact=True).shape == (0,)
    other = ops.WindingTree(*gpu(name, dev), levels=2)  # the exact sum does not read the tree
    assert torch.equal(ops.mesh_winding_number(p, other, exact=True), base)


# ---- c. node table ----
@pytest.mark.parametrize("name", ["sphere24", "torus32", "hand", "spanning"])
@pytest.mark.parametrize("L", [0, 1, None])
def test_node_table_matches_the_restatement(dev, name, L):
    vg, tg = gpu(name, dev)
    tree = ops.WindingTree(vg, tg, levels=L)
    ref = W.tree(name, L)
    assert tree.L == ref.L and tree.nodes.shape == ((8 ** (ref.L + 1) - 1) // 7, 8)
    assert np.array_equal(tree.leaf_ptr.cpu().numpy(), ref.leaf_ptr)
    assert np.array_equal(tree.face_order.cpu().numpy(), ref.order)
    assert torch.equal(tree.sorted_records[:, :, :3], vg[tg.long()][tree.face_order.long()])
    for l in range(ref.L + 1):
        lv, got = ref.levels[l], f64(tree.level(l))
        assert np.array_equal(tree.node_ranges(l).cpu().numpy(), np.stack([lv["begin"], lv["end"]], 1))
        occ = lv["r"] >= 0
        assert np.array_equal(got[:, 3] >= 0, occ) and (got[~occ, 3] == -1).all()
        bar_n, bar_c, bar_r = ref.bars(l)
        err_n = np.abs(got[:, 0:3] - lv["N"]).max(1)
        err_c = np.abs(got[:, 4:7] - lv["c"]).max(1)[occ]
        err_r = np.abs(got[:, 3] - lv["r"])[occ]
        print(f"{name} L={ref.L} level {l}: {occ.sum()} of {len(occ)} nodes occupied; N {np.max(err_n / np.maximum(bar_n, 1e-300)):.3f}, "
              f"c {err_c.max() / bar_c:.3f}, r {err_r.max() / bar_r:.3f} of their bars")
        assert (err_n <= bar_n).all() and (err_c <= bar_c).all() and (err_r <= bar_r).all()
    again = ops.WindingTree(vg, tg, levels=L)
    assert torch.equal(again.nodes, tree.nodes) and torch.equal(again.sorted_records, tree.sorted_records)
    assert torch.equal(again.leaf_ptr, tree.leaf_ptr)


# ---- d. fast against the restatement of the same tree ----
@pytest.mark.parametrize("name,L", [("sphere24", 3), ("sphere24", 1), ("torus32", 3), ("torus32", 1), ("hand", 1),
                                    ("two_clusters", 1), ("spanning", 1)])
@pytest.mark.parametrize("beta", [2.0, 3.0])
def test_fast_matches_the_restatement_of_the_same_tree(dev, name, L, beta):
    check_fast(dev, name, L, beta, cap=0.05)


@pytest.mark.parametrize("name", ["sphere24", "torus32", "spanning"])
@pytest.mark.parametrize("beta", [2.0, 3.0])
def test_fast_at_the_default_depth(dev, name, beta):
    assert W.default_levels(len(W.mesh(name)[1])) == {"sphere24": 5, "torus32": 5, "spanning": 2}[name]
    check_fast(dev, name, None, beta, cap=None)


def check_fast(dev, name, L, beta, cap):
    pts, w, away, _ = W.case(name)
    wf, margin, method_err = W.fast_case(name, L, beta)
    tree = ops.WindingTree(*gpu(name, dev), levels=L)
    p = torch.from_numpy(pts).to(dev)
    got_t = ops.mesh_winding_number(p, tree, beta=beta)
    got = f64(got_t)
    sure = (margin > 1e-4) & away
    print(f"{name} L={tree.L} beta={beta}: method error {method_err:.3e}; max |fast - restatement| = "
          f"{np.abs(got - wf)[sure].max():.3e} on {sure.mean():.4f} of the points; max |fast - exact| = "
          f"{np.abs(got - w)[away].max():.3e}")
    assert tree.L == W.tree(name, L).L
    assert cap is None or (~sure).mean() <= cap
    assert (np.abs(got - wf)[sure] <= BAR).all()
    assert method_err > 4 * BAR  # a case whose method error drowns in fp32 rounding says nothing here
    assert (np.abs(got - w)[away] <= 1.5 * method_err).all()
    decided = away & (np.abs(w - 0.5) > 2 * method_err)
    inside = ops.mesh_contains(p, tree, beta=beta).cpu().numpy()
    assert inside.dtype == np.bool_ and np.array_equal(inside[decided], (w > 0.5)[decided])
    # bit-identical under a permutation of the points and with the cell-order sort
    perm = torch.from_numpy(np.random.default_rng(23).permutation(len(pts))).to(dev)
    for cell_order in (False, True):
        assert torch.equal(ops.mesh_winding_number(p[perm], tree, beta=beta, cell_order=cell_order), got_t[perm])
        assert torch.equal(ops.mesh_winding_number(p, tree, beta=beta, cell_order=cell_order), got_t)


@pytest.mark.parametrize("name", ["sphere24", "hand", "two_clusters"])
def test_fast_falls_back_to_the_pair_sum(dev, name):
    pts, w, away, _ = W.case(name)
    p = torch.from_numpy(pts).to(dev)
    # L = 0, the points inside the root's beta r: the one leaf is summed
    root = W.tree(name, 0).levels[0]
    near = np.linalg.norm(pts.astype(np.float64) - root["c"][0], axis=1) < 0.99 * 2.0 * root["r"][0]
    assert near.sum() >= 100
    got = f64(ops.mesh_winding_number(p, ops.WindingTree(*gpu(name, dev), levels=0), beta=2.0))
    assert (np.abs(got - w)[near & away] <= BAR).all()
    # a beta no node passes: every leaf is summed, at any depth
    for L, beta in ((None, 1e30), (2, 1e30), (1, float("inf"))):
        got = f64(ops.mesh_winding_number(p, ops.WindingTree(*gpu(name, dev), levels=L), beta=beta))
        print(f"{name} L={L} beta={beta}: max |fast - exact| = {np.abs(got - w)[away].max():.3e}")
        assert (np.abs(got - w)[away] <= BAR).all()
    bad = torch.tensor([[0.0, float("nan"), 0.0], [float("inf"), 0.0, 0.0]], device=dev)
    tree = ops.WindingTree(*gpu(name, dev))
    for cell_order in (False, True):
        mixed = ops.mesh_winding_number(torch.cat([p[:70], bad, p[70:100]]), tree, cell_order=cell_order)
        assert torch.isnan(mixed[70:72]).all()
        assert torch.equal(torch.cat([mixed[:70], mixed[72:]]), ops.mesh_winding_number(p[:100].contiguous(), tree))


# ---- e. signed distance ----
def test_signed_distance_on_the_sphere(dev):
    v, t = W.mesh("sphere24")
    vg, tg = gpu("sphere24", dev)
    rng = np.random.default_rng(31)
    pts = rng.uniform(-0.95, 0.95, (3000, 3)).astype(np.float32)
    r_out = np.linalg.norm(v.astype(np.float64), axis=1).max()  # the vertices lie on the sphere, the facets sag inside
    r_in = np.sqrt(W.surface_d2(np.zeros((1, 3)), v, t)[0])
    assert 0 < r_out - r_in < 0.01
    p = torch.from_numpy(pts).to(dev).requires_grad_(True)
    vv = vg.clone().requires_grad_(True)
    mesh = Mesh(vv, tg)
    sd = mesh.signed_distance(p)
    assert sd.shape == (3000,) and sd.dtype == torch.float32
    assert torch.equal(sd.detach(), ops.mesh_signed_distance(p.detach(), vg, tg))  # trees built inside the call
    norm = np.linalg.norm(pts.astype(np.float64), axis=1)
    s = f64(sd.detach())
    assert (s[norm < r_in] < 0).all() and (s[norm > r_out] > 0).all() and (norm < r_in).sum() > 200
    assert np.abs(np.abs(s) - np.abs(norm - r_out)).max() <= (r_out - r_in) + 1e-5  # |sd| is the distance to the facets
    # gradient with the face and the sign fixed, against float64 autograd
    # Every point takes part.  The tolerance is the distance backward's 1e-4 of the gradient's max-abs, plus what fp32
    # allows sign (p - c) / d to be: c = sum b_k v_k carries three roundings of a unit-size coordinate (2^-24 each), the
    # difference one more, over three axes about 8 * 2^-24 in norm -- divided by d.  A point 1e-3 from a facet gets
    # 5e-4, one 0.02 away 2e-5; a vertex collects the terms of the points whose face it belongs to.
    wts = rng.uniform(-1, 1, 3000).astype(np.float32)
    (torch.from_numpy(wts).to(dev) * sd).sum().backward()
    face = mesh.closest_point(p.detach())[1].cpu().numpy()
    sign = np.sign(s)
    assert (np.abs(s) > 0).all()
    P = torch.tensor(pts, dtype=torch.float64, requires_grad=True)
    V = torch.tensor(v, dtype=torch.float64, requires_grad=True)
    corner = [V[torch.from_numpy(t[face, k].astype(np.int64))] for k in range(3)]
    (torch.tensor(wts * sign, dtype=torch.float64) * D.closest_point(P, *corner)[0].sqrt()).sum().backward()
    near = np.abs(wts) * 8 * 2.0 ** -24 / np.abs(s)
    bar_p = 1e-4 * P.grad.abs().max().item() + near
    bar_v = np.full(len(v), 1e-4 * V.grad.abs().max().item())
    np.add.at(bar_v, t[face].reshape(-1), np.repeat(near, 3))
    for name, got, want, bar in (("grad_points", p.grad, P.grad, bar_p), ("grad_v_pos", vv.grad, V.grad, bar_v)):
        err = (got.cpu().double() - want).abs().max(1)[0].numpy()
        print(f"{name}: max |got - float64| = {err.max():.3e} ({(err / bar).max():.3f} of its bar; max-abs "
              f"{want.abs().max().item():.3f}, smallest |sd| {np.abs(s).min():.2e})")
        assert (err <= bar).all()
    length = np.linalg.norm(f64(p.grad), axis=1) / np.abs(wts)
    assert (np.abs(length - 1) <= 1e-4 + near / np.abs(wts)).all()  # sign (p - c) / d is a unit vector


def test_signed_distance_gradient_is_zero_on_the_surface_and_open_meshes_run(dev):
    v, t = W.mesh("sphere24")
    vg, tg = gpu("sphere24", dev)
    on = np.concatenate([v[:40], v[t[:40]].mean(1), np.array([[0.1, 0.2, 0.3]], np.float32)]).astype(np.float32)
    q = torch.from_numpy(on).to(dev).requires_grad_(True)
    vv = vg.clone().requires_grad_(True)
    sd = ops.mesh_signed_distance(q, vv, tg)
    sd.sum().backward()
    zero = (sd.detach() == 0).cpu().numpy()
    assert zero[:40].all() and zero.sum() >= 40 and not zero[-1]
    assert torch.isfinite(q.grad).all() and torch.isfinite(vv.grad).all()
    assert (q.grad[torch.from_numpy(zero).to(dev)] == 0).all() and (q.grad[-1] != 0).any()
    # an open mesh with a degenerate face, a non-manifold edge and an unreferenced vertex
    pts = torch.from_numpy(W.case("hand")[0]).to(dev).requires_grad_(True)
    hand = Mesh(*gpu("hand", dev))
    sd = hand.signed_distance(pts)
    sd.sum().backward()
    assert torch.isfinite(sd).all() and torch.isfinite(pts.grad).all()
    w = hand.winding_number(pts.detach())
    assert torch.equal(sd.detach() < 0, (w > 0.5) & (sd.detach() != 0))
    assert torch.equal(hand.contains(pts.detach()), w > 0.5)


# ---- f. the extractor's orientation ----
def test_mesh_contains_pins_the_marching_cubes_orientation(dev):
    ax = torch.linspace(0, 1, 16, device=dev)
    grid = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1)
    level = (grid - 0.5).norm(dim=-1) - 0.3  # negative inside, the field's convention
    v, t = ops.marching_cubes(level.contiguous())
    lo, hi = float(v.min()), float(v.max())
    mesh = Mesh(v, t)
    c = 0.5
    probes = torch.tensor([[c, c, c], [c + 0.1, c - 0.1, c + 0.05], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.0, 1.0, 0.0],
                           [1.0, 0.0, 1.0], [c, c, c + 0.45]], device=dev)
    w = mesh.winding_number(probes, exact=True)
    print(f"marching cubes 16^3: T {t.shape[0]}, box {lo:.3f}..{hi:.3f}, w = {w.cpu().numpy()}")
    assert torch.allclose(w, torch.tensor([1.0, 1, 0, 0, 0, 0, 0], device=dev), atol=1e-4)
    assert mesh.contains(probes).tolist() == [True, True, False, False, False, False, False]
    low = mesh.simplify(grid=8)  # simplify keeps the orientation
    assert low.contains(probes).tolist() == [True, True, False, False, False, False, False]
    assert (mesh.signed_distance(probes)[:2] < 0).all() and (mesh.signed_distance(probes)[2:] > 0).all()


def test_mesh_contains_pins_the_marching_tetrahedra_orientation(dev):
    grid = ops.TetGrid(*(x.to(dev) for x in kuhn_tet_grid(16)))  # the unit cube, six Kuhn tets per cell
    level = (grid.vertices - 0.5).norm(dim=-1) - 0.3  # negative inside
    v, t = ops.marching_tets(grid.vertices, level.contiguous(), grid)
    mesh = Mesh(v, t)
    c = 0.5
    probes = torch.tensor([[c, c, c], [c + 0.1, c - 0.1, c + 0.05], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.0, 1.0, 0.0],
                           [1.0, 0.0, 1.0], [c, c, c + 0.45]], device=dev)
    w = mesh.winding_number(probes, exact=True)
    print(f"marching tetrahedra 16^3: T {t.shape[0]}, w = {w.cpu().numpy()}")
    assert torch.allclose(w, torch.tensor([1.0, 1, 0, 0, 0, 0, 0], device=dev), atol=1e-4)
    assert mesh.contains(probes).tolist() == [True, True, False, False, False, False, False]
    assert (mesh.signed_distance(probes)[:2] < 0).all() and (mesh.signed_distance(probes)[2:] > 0).all()


# ---- argument errors the host tests cannot reach (the device is checked before the shape) ----
def test_wrong_shapes_and_mismatched_arguments(dev):
    vg, tg = gpu("sphere24", dev)
    tree = ops.WindingTree(vg, tg)
    good = torch.zeros(4, 3, device=dev)
    for bad in (torch.zeros(4, 2, device=dev), torch.zeros(4, 3, 1, device=dev), torch.zeros(3, device=dev)):
        for call in (lambda p: ops.mesh_winding_number(p, tree), lambda p: ops.mesh_winding_number(p, tree, exact=True),
                     lambda p: ops.mesh_winding_number(p, vg, tg, exact=True), lambda p: ops.mesh_contains(p, tree),
                     lambda p: ops.mesh_signed_distance(p, vg, tg, tree=tree), lambda p: Mesh(vg, tg).contains(p)):
            with pytest.raises(ValueError):
                call(bad)
    with pytest.raises(TypeError):
        ops.mesh_winding_number(good.double(), tree)
    for bad_v in (torch.zeros(5, 2, device=dev), torch.zeros(5, 3, 1, device=dev)):
        with pytest.raises(ValueError):
            ops.WindingTree(bad_v, tg)
        with pytest.raises(ValueError):
            ops.mesh_winding_number(good, bad_v, tg, exact=True)
    for bad_t in (torch.zeros(6, 4, dtype=torch.int32, device=dev), torch.zeros(6, dtype=torch.int32, device=dev),
                  torch.zeros(6, 3, device=dev)):
        with pytest.raises(TypeError):  # the index-table check of the mesh stage
            ops.WindingTree(vg, bad_t)
        with pytest.raises(TypeError):
            ops.mesh_winding_number(good, vg, bad_t, exact=True)
    with pytest.raises(ValueError):  # an index outside the vertices, an empty mesh
        ops.WindingTree(vg[:10].contiguous(), tg)
    with pytest.raises(ValueError):
        ops.mesh_winding_number(good, vg[:10].contiguous(), tg, exact=True)
    with pytest.raises(ValueError):
        ops.WindingTree(vg, tg[:0])
    with pytest.raises(ValueError):  # a tree goes without t_pos_idx
        ops.mesh_winding_number(good, tree, tg)
    with pytest.raises(ValueError):
        ops.mesh_contains(good, tree, tg, exact=True)
    other = ops.WindingTree(vg[:-1].contiguous(), tg.clamp(max=vg.shape[0] - 2))  # built for another V
    with pytest.raises(ValueError):
        ops.mesh_signed_distance(good, vg, tg, tree=other)
    with pytest.raises(ValueError):
        ops.mesh_signed_distance(good, vg, tg, tg=ops.TriangleGrid(vg[:-1].contiguous(), tg.clamp(max=vg.shape[0] - 2)))
    with pytest.raises(TypeError):
        ops.mesh_signed_distance(good, vg, tg, tree=ops.TriangleGrid(vg, tg))
    with pytest.raises(ValueError):
        ops.mesh_winding_number(good, tree, beta=0.0)


# ---- g. the drop-ins ----
def test_drop_ins_match_the_restatement(dev, tmp_path):
    v, t = W.mesh("sphere24")
    stretched = v.astype(np.float64) * np.array([1.0, 0.6, 0.8]) + np.array([0.3, -0.2, 0.1])
    path = tmp_path / "guide.obj"
    with open(path, "w") as fh:
        fh.write("".join(f"v {x!r} {y!r} {z!r}\n" for x, y, z in stretched.tolist()))
        fh.write("".join(f"f {a + 1} {b + 1}//{b + 1} {c + 1}/{c + 1}\n" if i % 2 else f"f {a + 1} {b + 1} {c + 1}\n"
                         for i, (a, b, c) in enumerate(t.tolist())))
    loss_fn = shape.ShapeLoss(str(path))
    obj = loss_fn.sketchshape
    assert (loss_fn.mesh_scale, loss_fn.proximal_surface, loss_fn.delta) == (0.7, 0.3, 0.2)
    want_v = W.shape_loss_mesh(stretched)
    assert np.abs(obj.v - want_v).max() <= 1e-14 and np.array_equal(obj.f, t)
    half = shape.MeshOBJ(stretched, t.astype(np.int64)).normalize_mesh()
    assert abs(np.linalg.norm(half.v, axis=1).max() - 0.5) <= 1e-14 and np.abs(half.v.mean(0)).max() <= 1e-14
    v32 = obj.v.astype(np.float32)  # what the GPU holds
    rng = np.random.default_rng(41)
    xyz = rng.uniform(-1, 1, (3, 500, 3)).astype(np.float32)
    flat = xyz.reshape(-1, 3)
    w_ref = W.exact(flat, v32, t)
    d2_ref = W.surface_d2(flat, v32, t)
    tree = W.Tree(v32, t, W.default_levels(len(t)))
    wf, margin = W.fast(tree, flat, 2.0)
    away = np.sqrt(d2_ref) >= W.NEAR_SURFACE * tree.ext
    method_err = float(np.abs(wf - w_ref)[away].max())
    q = torch.from_numpy(xyz).to(dev)
    # MeshOBJ.winding_number
    w = obj.winding_number(q)
    assert w.shape == (3, 500) and w.device == q.device and w.dtype == torch.float32
    assert (np.abs(f64(w).reshape(-1) - w_ref)[away] <= 1.5 * method_err).all()
    # MeshOBJ.gaussian_weighted_distance: d within 4e-6 of the mesh's size (tests/test_gpu_mesh_distance.py), so
    # |d(d2)| <= 2 d 4e-6 Lm + ..., through exp(-d2 / 2 sigma^2) whose slope is at most 1 / (2 sigma^2); + fp32 exp rounding
    sigma = 0.3
    g = obj.gaussian_weighted_distance(q, sigma)
    assert g.shape == (3, 500) and g.device == q.device
    dw_bar = (2 * np.sqrt(d2_ref) + 1e-5) * 4e-6 * 2.0 / (2 * sigma ** 2) + 4 * 2.0 ** -23
    err = np.abs(f64(g).reshape(-1) - W.gaussian_weight(d2_ref, sigma))
    print(f"drop-ins: method error {method_err:.3e}; weight error {err.max():.3e} ({(err / dw_bar).max():.3f} of its bar)")
    assert (err <= dw_bar).all()
    # ce_pq_loss
    p64 = torch.from_numpy(rng.uniform(0, 1.1, (40, 5))).to(dev)
    q64 = torch.from_numpy((rng.uniform(0, 1, 200) > 0.5).astype(np.float64)).to(dev)
    wt64 = torch.from_numpy(rng.uniform(0, 1, 200)).to(dev)
    for wt in (None, wt64):
        want = W.ce_pq(f64(p64).reshape(-1), f64(q64), None if wt is None else f64(wt))[0]
        assert abs(shape.ce_pq_loss(p64, q64, wt).item() - want) <= 1e-10 * abs(want)
    # ShapeLoss.forward: the points within the method error of 0.5 are left out on both sides
    keep = np.abs(w_ref - 0.5) > 2 * method_err
    assert (~keep).mean() <= 0.05
    sig = rng.uniform(-2, 30, 1500).astype(np.float32)
    xk = torch.from_numpy(flat[keep]).to(dev).requires_grad_(True)
    sk = torch.from_numpy(sig[keep]).to(dev).requires_grad_(True)
    loss = loss_fn(xk, sk)
    loss.backward()
    assert xk.grad is None and sk.grad is not None and loss.dim() == 0
    ind = (w_ref > 0.5)[keep]
    want, want_g = W.shape_loss(ind, d2_ref[keep], sig[keep])
    s64 = sig[keep].astype(np.float64)
    occ = np.clip(1 - np.exp(-0.2 * s64), 0, 1.1)
    ce0, dp0 = W.ce_pq(occ, ind.astype(np.float64))  # unweighted: what an error of the weight multiplies
    ce_each = -(occ * np.log(np.clip(ind, 1e-4, 1 - 1e-4)) + (1 - occ) * np.log(np.clip(1.0 - ind, 1e-4, 1 - 1e-4)))
    eps = 2.0 ** -23
    loss_bar = (np.abs(ce_each) * dw_bar[keep]).sum() + 32 * eps * np.abs(ce_each).sum()
    print(f"ShapeLoss: {keep.sum()} points, loss {loss.item():.6f} want {want:.6f}, |diff| {abs(loss.item() - want):.3e} "
          f"(bar {loss_bar:.3e})")
    assert abs(loss.item() - want) <= loss_bar
    docc = 0.2 * np.exp(-0.2 * s64) * ((1 - np.exp(-0.2 * s64)) >= 0)
    g_bar = np.abs(dp0 * docc) * dw_bar[keep] + 32 * eps * np.abs(want_g) + 1e-12
    g_err = np.abs(f64(sk.grad) - want_g)
    print(f"ShapeLoss: gradient error at most {(g_err / g_bar).max():.3f} of its bar, max |g| {np.abs(want_g).max():.3e}")
    assert (g_err <= g_bar).all()
