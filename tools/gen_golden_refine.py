"""tools/gen_golden_refine.py -- AUTHORING ONLY, CPU (never imported by tests, bench or smoke): records tests/golden/golden_refine.npz
from the reference's own refine-and-upsample front: data_utils/mirror_partial.py (mirror_and_concat), models/point_upsample_module.py
(point_upsample) and dpsr_evaluation.py (shapenet_psr_normalize, network_output_to_dpsr_grid with a stub `dpsr`).  The reference
modules are imported where they lie, through tools/ref_shims.py and the stub loader of tools/gen_golden_dpsr.py; nothing is copied.

(a) The kernel cases of tests/refine_cases.py (inputs are regenerated from their seeds, not stored):
  mirror_<case>_out, _center      mirror_and_concat(...)[0] and the torch.mean centre it used; the permutation is torch.randperm under
                                  torch.manual_seed(MIRROR_PERM_SEED), recorded as mirror_<case>_perm
  refine_<case>_points, _normals  network_output_to_dpsr_grid's refined points / normals;  _bbox: min / max of point_upsample's xyz
                                  (the big case records the rows refine_cases.big_rows only: the whole of it exceeds the fixture's size)
(b) One network case: the shipped ..._s3_noise_0.02_symmetry configuration reduced (NET_ARCH), weights from synth_state_dict:
  net_config_json, net_spec_names, net_spec_shapes, net_x (2, 40, 6), net_label, net_perm, net_X (2, 80, 7) the mirrored input,
  net_disp the reference's displacement, net_points / net_normals its refined points / normals, net_fps_margin.
The smallest relative gap between the farthest and the second farthest candidate over every FPS step of the network case is printed.
A mirrored cloud holds pairs of points that are exact twins on the two untouched axes, so exact ties occur whatever the seed (margin
0): the reference's kernel, the oracle and the HIP kernel all resolve a tie to the lowest index.  Among the strict steps, prefer a
--net_seed whose margin is wide (a float32 rounding must not change a selection).

usage:  python tools/gen_golden_refine.py [--reference DIR] [--net_seed 0] [--out tests/golden]
"""
import argparse
import copy
import json
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_CAP = 200 * 1024
NET_ARCH = {"npoint": [40, 20, 10, 5], "nsample": [8, 8, 8, 8], "K": 4, "feature_dim": [16, 32, 32, 64, 64],
            "decoder_feature_dim": [32, 32, 32, 64, 64]}
NET_B, NET_N = 2, 40
SYMMETRY_CFG = ("pointnet2/configs/shapenet_psr_configs/refine_and_upsample_configs/"
                "config_refine_and_upsample_standard_attention_s3_noise_0.02_symmetry.json")


def load_reference(ref_root):
    """the reference's mirror_partial, point_upsample_module and dpsr_evaluation modules"""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    sys.path.insert(0, REPO)
    import ref_shims
    ref_shims.REF = ref_root
    ref_shims.install()
    import gen_golden_dpsr
    gen_golden_dpsr.load_reference(ref_root)  # (stubs for trimesh, skimage, igl, ...; dpsr_utils from the reference)
    for name in ("matplotlib", "matplotlib.pyplot"):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)
                sys.modules[name].use = lambda *a, **k: None
    if not hasattr(sys.modules["matplotlib"], "pyplot"):
        sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    # what dpsr_utils/io_utils.py imports to write files; nothing here writes one
    for name, attrs in (("pytorch3d.io", ()), ("pyntcloud", ("PyntCloud",)), ("pandas", ())):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)
                for a in attrs:
                    setattr(sys.modules[name], a, None)
    sys.modules["pytorch3d"].io = sys.modules["pytorch3d.io"]
    import data_utils.mirror_partial as MP
    import models.point_upsample_module as PU
    import dpsr_evaluation as DE
    for m in (MP, PU, DE):
        assert os.path.abspath(m.__file__).startswith(os.path.abspath(ref_root)), m.__file__
    return MP, PU, DE


def fps_margin(xyz, npoints):
    """plain FPS from index 0 in float64 over the chain of levels -> the smallest (best - second) / best over every step"""
    worst = np.inf
    cur = np.asarray(xyz, np.float64)
    for m in npoints:
        d = np.full(len(cur), 1e10)
        sel = [0]
        for _ in range(1, m):
            d = np.minimum(d, ((cur - cur[sel[-1]]) ** 2).sum(1))
            order = np.argsort(d)
            best, second = d[order[-1]], d[order[-2]]
            worst = min(worst, (best - second) / best)
            sel.append(int(order[-1]))
        cur = cur[sel]
    return worst


def kernel_cases(MP, PU, DE, out):
    import torch
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import refine_cases as RC
    for name, c in RC.MIRROR_CASES.items():
        x = torch.from_numpy(RC.mirror_inputs(name))
        torch.manual_seed(RC.MIRROR_PERM_SEED)
        got = MP.mirror_and_concat(x, axis=c["axis"], num_points=[], attach_label=c["label"], permute=c["perm"])[0]
        out["mirror_%s_out" % name] = got.numpy()
        out["mirror_%s_center" % name] = torch.mean(x[:, :, 0:3], dim=1).numpy()
        if c["perm"]:
            torch.manual_seed(RC.MIRROR_PERM_SEED)
            perm = torch.randperm(2 * c["N"])
            g = torch.Generator(device="cpu")
            g.manual_seed(RC.MIRROR_PERM_SEED)
            assert torch.equal(perm, torch.randperm(2 * c["N"], generator=g))  # slide_amd.refine.refine_permutation
            out["mirror_%s_perm" % name] = perm.numpy().astype(np.int32)
    for name, c in RC.REFINE_CASES.items():
        X, disp = (torch.from_numpy(a) for a in RC.refine_inputs(name))
        first, center = RC.form_flags(c["form"])
        cfg = {"point_upsample_factor": c["factor"], "include_displacement_center_to_final_output": center,
               "output_scale_factor": c["out_scale"], "first_refine_coarse_points": first}
        _, pts, nrm = DE.network_output_to_dpsr_grid(X, disp, lambda p, n: None, c["scale"], cfg, last_dim_as_indicator=c["ldx"] == 7,
                                                     only_original_points_split=c["only_orig"], explicit_normalize=c["mode"] == "normalize")
        rows = c["M"] // 2 if c["only_orig"] else c["M"]
        child = PU.point_upsample(X[:, :rows, 0:6], disp[:, :rows], c["factor"], include_displacement_center_to_final_output=center,
                                  output_scale_factor_value=c["out_scale"], first_refine_coarse_points=first)
        bbox = torch.stack([child[:, :, 0:3].min(dim=1)[0], child[:, :, 0:3].max(dim=1)[0]], dim=1)
        pts, nrm = pts.numpy(), nrm.numpy()
        assert pts.dtype == np.float32 and pts.shape == (c["B"], RC.out_rows(c), 3), (name, pts.shape)
        if name == RC.BIG:
            sel = RC.big_rows(pts.shape[1])
            pts, nrm = pts[:, sel], nrm[:, sel]
        out["refine_%s_points" % name], out["refine_%s_normals" % name] = np.ascontiguousarray(pts), np.ascontiguousarray(nrm)
        out["refine_%s_bbox" % name] = bbox.numpy()
        print("  %-22s rows %5d  zeros %4d  0.99s %4d" % (name, RC.out_rows(c), int((pts == 0).sum()), int((pts == np.float32(0.99)).sum())))


def network_case(MP, PU, DE, ref_root, seed, out):
    import torch
    import gen_golden as G
    cfg = G.load_cfg(os.path.join(ref_root, SYMMETRY_CFG))
    hp = cfg["pointnet_config"]
    for k in ("npoint", "nsample", "feature_dim", "decoder_feature_dim", "K"):
        hp["architecture"][k] = copy.deepcopy(NET_ARCH[k])
    out["net_config_json"] = np.array(json.dumps(hp))  # (before the constructor edits it in place)
    net, spec = G.build_net(cfg)
    out["net_spec_names"], out["net_spec_shapes"] = G.spec_arrays(spec)
    rs = np.random.RandomState(seed)
    x = np.zeros((NET_B, NET_N, 6), np.float32)
    x[:, :, 0:3] = (0.4 * rs.standard_normal((NET_B, NET_N, 3))).astype(np.float32)
    n = rs.standard_normal((NET_B, NET_N, 3))
    x[:, :, 3:6] = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(np.float32)
    label = np.array([0, 4], np.int64)
    torch.manual_seed(seed)
    perm = torch.randperm(2 * NET_N)
    torch.manual_seed(seed)
    X = MP.mirror_and_concat(torch.from_numpy(x), axis=2, num_points=[], attach_label=True, permute=True)[0]
    with torch.no_grad():
        disp = net(X, None, ts=None, label=torch.from_numpy(label))
        _, pts, nrm = DE.network_output_to_dpsr_grid(X, disp, lambda p, q: None, 1, hp, last_dim_as_indicator=True,
                                                     only_original_points_split=False, explicit_normalize=True)
    margin = min(fps_margin(X[b, :, 0:3].numpy(), NET_ARCH["npoint"]) for b in range(NET_B))
    out.update(net_x=x, net_label=label, net_perm=perm.numpy().astype(np.int32), net_X=X.numpy(), net_disp=disp.numpy(),
               net_points=pts.numpy(), net_normals=nrm.numpy(), net_fps_margin=np.float64(margin), net_seed=np.int64(seed))
    print("  network case: params %d, displacement %s rms %.3f, smallest FPS selection margin %.3e"
          % (sum(int(np.prod(s)) for _, s in spec), tuple(disp.shape), float(np.sqrt((disp.numpy() ** 2).mean())), margin))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="root of the reference tree (default: tools/ref_shims.REF)")
    ap.add_argument("--net_seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    a = ap.parse_args()
    if a.reference is None:
        sys.path.insert(0, os.path.join(REPO, "tools"))
        import ref_shims
        a.reference = ref_shims.REF
    MP, PU, DE = load_reference(a.reference)
    out = {}
    kernel_cases(MP, PU, DE, out)
    network_case(MP, PU, DE, a.reference, a.net_seed, out)
    path = os.path.join(a.out, "golden_refine.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote %s (%d bytes, cap %d)" % (path, size, SIZE_CAP))
    assert size <= SIZE_CAP, "the fixture exceeds the cap"


if __name__ == "__main__":
    main()
