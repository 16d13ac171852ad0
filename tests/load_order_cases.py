"""The cases of tests/test_gpu_load_order.py, shared with tests/golden/make_load_order_golden.py (which ran them on the
build BEFORE the loads of the per-Gaussian forward kernels were rescheduled and stored every output).

Every runner returns {name: numpy array}; the inputs are seeded, so the generator and the test feed the same bits.  Device
tensors are allocated at exactly P rows: a load that is issued for the lanes past the end of the last wave has to be clamped."""
import ctypes as C
import os

import numpy as np
import torch

from oracle import rasterizer_oracle as O
from rodygs_amd import _lib
from rodygs_amd.rasterizer import _c_settings

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W, H, SEED = 64, 48, 5
PRE_BLOCK, REC_BYTES = 256, 64          # RDG_PRE_BLOCK, sizeof(RdgRec)


def geom_layout(P):
    """Byte offsets of the `geom` workspace: rdg_geom_layout (csrc/rdg_common.h) restated."""
    up = lambda v: (v + 255) // 256 * 256   # noqa: E731
    Pp = max(P, 1)
    nblk = (Pp + PRE_BLOCK - 1) // PRE_BLOCK
    L, o = {}, 0
    L["rec"] = o; o = up(o + Pp * REC_BYTES)                # noqa: E702
    L["tiles_touched"] = o; o = up(o + Pp * 4)              # noqa: E702
    L["clamped"] = o; o = up(o + Pp)                        # noqa: E702
    L["block_sums"] = o; o = up(o + (nblk + 1) * 4)         # noqa: E702
    L["rectd"] = o; o = up(o + Pp * 16)                     # noqa: E702
    L["total"], L["nblk"] = o, nblk
    return L


# ---- projection (rdg_preprocess_fwd_kernel<false>) ---------------------------------------------------------------
# name -> (P, SH degree, variant)
PROJECTION_CASES = {f"proj_p{P}_deg3": (P, 3, "shs") for P in (1, 63, 65, 257, 1000)}
PROJECTION_CASES.update({f"proj_p257_deg{d}": (257, d, "shs") for d in (0, 1, 2)})
PROJECTION_CASES["proj_p257_colors"] = (257, 3, "colors")
PROJECTION_CASES["proj_p257_cov3d"] = (257, 3, "cov3d")


def _cov3d(scales, rots):
    """[P,6] upper triangle of R diag(s)^2 R^T (any values would do: the kernel only reads them)."""
    q = rots / rots.norm(dim=1, keepdim=True)
    r, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    Lm = R * scales.unsqueeze(1)
    S = Lm @ Lm.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], dim=1).contiguous()


def run_projection(name, dev="cuda"):
    import hip_stages as HS
    P, deg, variant = PROJECTION_CASES[name]
    sc = O.synthetic_scene(P, W, H, deg, seed=SEED)
    L = _lib.lib()
    rs = HS.make_settings(sc, deg, dev=dev)
    d = lambda t: t.to(dev).contiguous().clone()   # noqa: E731  (an allocation of its own, exactly P rows)
    m3, op, vm, pm = d(sc["means3D"]), d(sc["opacities"]), d(sc["viewmatrix"]), d(sc["projmatrix"])
    shs = d(sc["shs"]) if variant != "colors" else None
    colors = None
    if variant == "colors":
        colors = d(torch.rand(P, 3, generator=torch.Generator().manual_seed(SEED + 1)))
    scl, rot, cov = d(sc["scales"]), d(sc["rotations"]), None
    if variant == "cov3d":
        cov, scl, rot = d(_cov3d(sc["scales"], sc["rotations"])), None, None
    cs = _c_settings(rs, P, sc["shs"].shape[1])
    lay = geom_layout(P)
    assert L.rdg_geom_bytes(P) == lay["total"], "geom layout restated wrongly"
    # 0xAB fill: a row the kernel does not write shows up as a difference, not as a lucky zero
    geom = torch.full((lay["total"],), 0xAB, dtype=torch.uint8, device=dev)
    radii = torch.full((P,), -7, dtype=torch.int32, device=dev)
    nren = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(L.rdg_preprocess_forward(C.byref(cs), _lib.ptr(m3), _lib.ptr(shs), _lib.ptr(colors), _lib.ptr(op),
                                        _lib.ptr(scl), _lib.ptr(rot), _lib.ptr(cov), _lib.ptr(vm), _lib.ptr(pm),
                                        _lib.ptr(geom), _lib.ptr(radii), _lib.ptr(nren), _lib.stream_ptr()), "preprocess")
    torch.cuda.synchronize()
    g = geom.cpu().numpy()
    cut = lambda key, n: g[lay[key]:lay[key] + n].copy()   # noqa: E731
    return {"rec": cut("rec", P * REC_BYTES), "tiles_touched": cut("tiles_touched", P * 4), "clamped": cut("clamped", P),
            "block_sums": cut("block_sums", (lay["nblk"] + 1) * 4), "rectd": cut("rectd", P * 16),
            "radii": radii.cpu().numpy(), "num_rendered": nren.cpu().numpy()}


# ---- a fully culled wave between visible ones (tests/hip_stages.run_stages) ---------------------------------------
CULLED_CASES = {"culled_behind_64_127": (slice(64, 128), "behind"), "culled_outside_x_0_63": (slice(0, 64), "outside_x")}
STAGE_KEYS = ("depth", "xy", "conic_opacity", "rgb", "normal", "tiles_touched", "radii", "keys_unsorted", "vals_unsorted",
              "keys_sorted", "vals_sorted", "ranges")


def culled_scene(name):
    rows, how = CULLED_CASES[name]
    sc = O.synthetic_scene(320, W, H, 3, seed=SEED)
    m = sc["means3D"].clone()
    if how == "behind":
        m[rows, 2] = -5.0
    else:
        m[rows, 0] = 50.0 * m[rows, 2]       # tan(half fov) < 1: far outside the frustum in x, in front of the camera
    sc["means3D"] = m
    return sc, rows


def run_culled(name, dev="cuda"):
    import hip_stages as HS
    sc, _ = culled_scene(name)
    out = HS.run_stages(sc, 3, dev=dev)
    res = {k: np.ascontiguousarray(out[k]) for k in STAGE_KEYS}
    res["D"] = np.array([out["D"]], dtype=np.int64)
    return res


# ---- dynamic getter (rdg_dyn_getter_fwd_kernel / rdg_dyn_getter_bwd_kernel) ----------------------------------------
GETTER_CASES = {f"getter_p{P}_tu{Tu}": (P, Tu, True) for P in (1, 1023, 1025, 2500) for Tu in (1, 7, 100)}
GETTER_CASES["getter_p1025_tu7_no_upstream"] = (1025, 7, False)
GETTER_SCALE = 1.7


def getter_file(name):
    """The stored outputs of the large clouds do not fit one file of the size a repository should hold: one per table size."""
    P, Tu, up = GETTER_CASES[name]
    return "G14_preprocess_getter_parent.npz" if (P == 1 or not up) else f"G14_preprocess_getter_parent_tu{Tu}.npz"


def run_getter(name, dev="cuda"):
    P, Tu, upstream = GETTER_CASES[name]
    g = torch.Generator().manual_seed(1000 * Tu + P)
    rn = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    xyz, scaling, rotation, opacity = rn(P, 3), 0.3 * rn(P, 3) - 2.0, rn(P, 4), 2.0 * rn(P, 1)
    coeff, bases = 0.5 * rn(P, 16), 0.2 * rn(Tu + 1, 16, 7)
    ti = torch.randint(0, Tu, (P,), generator=g, dtype=torch.int64)          # random birth indices
    ups = [rn(P, 3), rn(P, 3), rn(P, 4), rn(P, 1)] if upstream else [None] * 4
    order = torch.argsort(ti, stable=True)
    inv = torch.empty_like(order)
    inv[order] = torch.arange(P)
    seg = torch.searchsorted(ti[order].contiguous(), torch.arange(Tu + 1, dtype=torch.int64))
    L = _lib.lib()
    d = lambda t: None if t is None else t.to(dev).contiguous().clone()   # noqa: E731
    i32 = lambda t: t.to(torch.int32).to(dev).contiguous()   # noqa: E731
    x, s, r, o, c, b, t_ = d(xyz), d(scaling), d(rotation), d(opacity), d(coeff), d(bases), d(ti)
    gm, gsc, gr, go = (d(t) for t in ups)
    od, iv, sg = i32(order), i32(inv), i32(seg)
    f32 = dict(dtype=torch.float32, device=dev)
    nan = lambda *s: torch.full(s, float("nan"), **f32)   # noqa: E731
    means3D, scales, rots, opac = nan(P, 3), nan(P, 3), nan(P, 4), nan(P, 1)
    st = _lib.stream_ptr()
    _lib.check(L.rdg_dyn_getter_forward(P, Tu, _lib.ptr(c), _lib.ptr(t_), _lib.ptr(b), GETTER_SCALE, _lib.ptr(x), _lib.ptr(s),
                                        _lib.ptr(r), _lib.ptr(o), _lib.ptr(means3D), _lib.ptr(scales), _lib.ptr(rots),
                                        _lib.ptr(opac), st), "rdg_dyn_getter_forward")
    d_xyz, d_scaling, d_rotation, d_opacity, d_coeff = nan(P, 3), nan(P, 3), nan(P, 4), nan(P, 1), nan(P, 16)
    d_bases = nan(Tu + 1, 16, 7)
    sws = torch.full((L.rdg_deform_sorted_ws_bytes(P),), 0xAB, dtype=torch.uint8, device=dev)
    _lib.check(L.rdg_dyn_getter_backward(P, Tu, _lib.ptr(c), _lib.ptr(t_), _lib.ptr(b), GETTER_SCALE, _lib.ptr(s), _lib.ptr(r),
                                         _lib.ptr(o), _lib.ptr(gm), _lib.ptr(gsc), _lib.ptr(gr), _lib.ptr(go),
                                         _lib.ptr(d_xyz), _lib.ptr(d_scaling), _lib.ptr(d_rotation), _lib.ptr(d_opacity),
                                         _lib.ptr(d_coeff), _lib.ptr(d_bases), _lib.ptr(od), _lib.ptr(iv), _lib.ptr(sg),
                                         _lib.ptr(sws), st), "rdg_dyn_getter_backward")
    torch.cuda.synchronize()
    u8 = lambda t: t.cpu().numpy().view(np.uint8).reshape(-1).copy()   # noqa: E731  (bytes: NaN payloads compare too)
    return {"means3D": u8(means3D), "scales": u8(scales), "rots": u8(rots), "opac": u8(opac), "d_xyz": u8(d_xyz),
            "d_scaling": u8(d_scaling), "d_rotation": u8(d_rotation), "d_opacity": u8(d_opacity), "d_coeff": u8(d_coeff),
            "gs": sws[:P * 32].cpu().numpy().copy()}
