"""Times the texture bake (goi_hyperplane_amd/texture.py, csrc/texture.hip) and writes profiles/texture.json.  Two cases on
tools/field_time.py's 1 M-Gaussian scene (cameras on an orbit of radius 4 around it): its cleaned iso-surface at R = 128
decimated to 50 000 faces, rendered at 512^2 into a 1024^2 texture (the reference's sizes), and the same surface decimated to
2000 faces, rendered at 128^2 into a 256^2 texture.  Per stage, for one view (the ninth: 45 degrees from below):

    device   the stage on the device: median (min, max) over --rounds of windows of --iters calls between two device events,
             the stages ALTERNATING inside a round, after one warm-up round
    torch    the reference's stage restated in torch on the same device, where it has one: the grid put as gui/grid_put.py does
             it (the valid samples compacted with a boolean index, which synchronises; scatter_add_, float atomics: not
             reproducible; its early exit kept); device events like the device figure
    host     the reference's tail of main.py:727-749 as it stands: the texture and mask copied to the host, scipy's dilation
             and erosion, sklearn's kd-tree, the copy back; wall clock, best of --host-runs

render_gui (the Gaussian rasterizer, not part of this change) is timed for scale.  There is no torch counterpart for the
rasterizer; its row carries the time of the whole call (two memsets, both passes, the shading pass) and the bytes of its
64-bit atomicMin operations over that time: 8 bytes per covered sample, counted exactly with the numpy restatement for the
small case and bounded from below by the pixels hit for the large one.  `bake` is the whole 26-view loop with its one
read-back.  The accumulate_normalize row includes a clone of the texture and of its count per call (accumulate works in place).

    python tools/texture_time.py [--out profiles/texture.json] [--rounds 5] [--iters 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import field_time  # noqa: E402

P, R, NUM_BLOCKS, RELAX = 1_000_000, 128, 16, 1.5
CASES = ((50000, 512, 1024), (2000, 128, 256))  # target faces, render resolution, texture size
ORBIT_RADIUS, VIEW = 4.0, 9


def torch_linear_put(H, W, coords, values):
    """linear_grid_put_2d(return_count=True) with scatter_add_"""
    idx = (coords * 0.5 + 0.5) * torch.tensor([H - 1, W - 1], dtype=torch.float32, device=coords.device)
    i00 = idx.floor().long()
    i00[:, 0].clamp_(0, H - 2)
    i00[:, 1].clamp_(0, W - 2)
    h, w = idx[:, 0] - i00[:, 0].float(), idx[:, 1] - i00[:, 1].float()
    result = torch.zeros(H * W, values.shape[1], device=values.device)
    count = torch.zeros(H * W, 1, device=values.device)
    for di, dj, wt in ((0, 0, (1 - h) * (1 - w)), (0, 1, (1 - h) * w), (1, 0, h * (1 - w)), (1, 1, h * w)):
        flat = ((i00[:, 0] + di) * W + i00[:, 1] + dj).unsqueeze(1)
        result.scatter_add_(0, flat.repeat(1, values.shape[1]), values * wt.unsqueeze(1))
        count.scatter_add_(0, flat, wt.unsqueeze(1))
    return result.view(H, W, -1), count.view(H, W, 1)


def torch_grid_put(H, W, coords, values, valid, min_resolution):
    """mipmap_linear_grid_put_2d(return_count=True) as the reference runs it: compacted samples, the early exit"""
    F = torch.nn.functional
    coords, values = coords[valid], values[valid]
    result = torch.zeros(H, W, values.shape[1], device=values.device)
    count = torch.zeros(H, W, 1, device=values.device)
    cH, cW = H, W
    while min(cH, cW) > min_resolution:
        mask = count.squeeze(-1) == 0
        if not mask.any():
            break
        cur, cnt = torch_linear_put(cH, cW, coords, values)
        up = F.interpolate(cur.permute(2, 0, 1).unsqueeze(0).contiguous(), (H, W), mode="bilinear", align_corners=False)
        result[mask] = result[mask] + up.squeeze(0).permute(1, 2, 0).contiguous()[mask]
        upc = F.interpolate(cnt.view(1, 1, cH, cW), (H, W), mode="bilinear", align_corners=False)
        count[mask] = count[mask] + upc.view(H, W, 1)[mask]
        cH, cW = cH // 2, cW // 2
    return result, count


def host_fill(albedo, mask, radius=32):
    """gui/main.py:727-751"""
    from scipy.ndimage import binary_dilation, binary_erosion
    from sklearn.neighbors import NearestNeighbors
    a, m = albedo.cpu().numpy(), mask.cpu().numpy()
    inpaint = binary_dilation(m, iterations=radius)
    inpaint[m] = 0
    search = m.copy()
    search[binary_erosion(search, iterations=3)] = 0
    sc, ic = np.stack(np.nonzero(search), axis=-1), np.stack(np.nonzero(inpaint), axis=-1)
    if len(sc) and len(ic):
        _, ind = NearestNeighbors(n_neighbors=1, algorithm="kd_tree").fit(sc).kneighbors(ic)
        a[tuple(ic.T)] = a[tuple(sc[ind[:, 0]].T)]
    return torch.from_numpy(a).to(albedo.device)


def measure(args, dev):
    from goi_hyperplane_amd import _lib, field, mesh, render, texture
    from tests import texture_reference as ref
    _lib.load()
    m = field_time.model(P, dev)
    stub = field_time.Stub(m)
    shs = torch.zeros((P, 16, 3), device=dev)
    shs[:, 0, :] = (m["rgb"] - 0.5) / 0.28209479177387814
    pc = render.GaussianSet(m["xyz"], m["scaling"], torch.nn.functional.normalize(m["rotation"], dim=1), m["opacity"][:, None].contiguous(),
                            shs, torch.zeros((P, 16), device=dev))
    bg = torch.zeros(3, device=dev)
    f = field.density_grid(m["xyz"], m["opacity"], m["scaling"], m["rotation"], R, NUM_BLOCKS, RELAX)
    thresh = float(torch.quantile(f.occ.reshape(-1)[:: max(1, R ** 3 // 1_000_000)], 0.9))  # field_time.py's surface
    raw = field.extract_mesh(stub, thresh, R, NUM_BLOCKS, RELAX, colors=m["rgb"])
    cl = mesh.clean(raw.vertices, raw.faces, raw.colors)
    rows = []
    with torch.no_grad():
        for target, res, size in CASES:
            dec = mesh.decimate(cl.vertices, cl.faces, cl.colors, target_faces=target)
            geo = mesh.Mesh(dec.vertices, dec.faces, dec.colors, mesh.vertex_normals(dec.vertices, dec.faces), raw.center, raw.scale)
            F = int(geo.faces.shape[0])
            at = texture.atlas(F, size, faces=geo.faces)
            idx = at.vmapping.long()
            v, vn = geo.vertices[idx].contiguous(), geo.normals[idx].contiguous()
            cams = texture.orbit_cameras(res, radius=ORBIT_RADIUS)
            cam = render.TorchCamera(cams[VIEW], dev)
            rot = torch.tensor(np.ascontiguousarray(cams[VIEW].pose[:3, :3]), device=dev)
            image = render.render_gui(cam, pc, bg)["image"]
            v_clip = texture.clip_positions(v, cam.full_proj_transform)
            r = texture.rasterize(v_clip, at.ft, res, res)
            coords, values, valid = texture.resolve(r, at.vt, at.ft, vn, at.ft, rot, image)
            mr = size // 4
            cur, cur_cnt = texture.grid_put(size, size, coords, values, valid, mr, return_count=True)
            baked = texture.bake(pc, geo, bg, texture_size=size, render_resolution=res, cameras=cams)
            acc = torch.zeros((size, size, 3), device=dev)
            acc_cnt = torch.zeros((size, size, 1), device=dev)
            for c in cams:  # the texture before the fill, for the fill's timing
                tc = render.TorchCamera(c, dev)
                rr = texture.rasterize(texture.clip_positions(v, tc.full_proj_transform), at.ft, res, res)
                co, va, ok = texture.resolve(rr, at.vt, at.ft, vn, at.ft, torch.tensor(np.ascontiguousarray(c.pose[:3, :3]), device=dev),
                                             render.render_gui(tc, pc, bg)["image"])
                texture.accumulate(acc, acc_cnt, *texture.grid_put(size, size, co, va, ok, mr, return_count=True))
            normal, mask = texture.normalize(acc, acc_cnt)
            device = {
                "render_gui": lambda: render.render_gui(cam, pc, bg),
                "rasterize": lambda: texture.rasterize(v_clip, at.ft, res, res),
                "resolve": lambda: texture.resolve(r, at.vt, at.ft, vn, at.ft, rot, image),
                "grid_put": lambda: texture.grid_put(size, size, coords, values, valid, mr, return_count=True),
                "accumulate_normalize": lambda: (texture.accumulate(acc.clone(), acc_cnt.clone(), cur, cur_cnt), texture.normalize(acc, acc_cnt)),
                "fill": lambda: texture.fill(normal, mask, 32),
                "bake": lambda: texture.bake(pc, geo, bg, texture_size=size, render_resolution=res, cameras=cams),
                "torch_grid_put": lambda: torch_grid_put(size, size, coords, values, valid, mr),
            }
            times = {k: [] for k in device}
            for rnd in range(args.rounds + 1):
                for name, fn in device.items():
                    ms = field_time.window_ms(fn, 1 if name == "bake" else args.iters)
                    if rnd:
                        times[name].append(ms)
            best = None
            for _ in range(args.host_runs):
                torch.cuda.synchronize()
                t = time.perf_counter()
                filled = host_fill(normal, mask)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t
                best = dt if best is None else min(best, dt)
            n, cell = texture.atlas_grid(F, size)
            n_valid, hit = int(valid.sum()), int((r.tri > 0).sum())
            row = {"P": P, "R": R, "faces": F, "render_resolution": res, "texture_size": size, "atlas_cells": n, "atlas_cell_texels": cell,
                   "min_resolution": mr, "view": VIEW, "pixels_hit": hit, "valid_samples": n_valid,
                   "texels_reached_by_26_views": int(mask.sum()), "texels_filled": int((texture.fill(normal, mask, 32, return_index=True)[1] >= 0).sum())}
            for name, ts in times.items():
                row[name + "_ms"] = round(statistics.median(ts), 3)
                row[name + "_ms_min_max"] = [round(min(ts), 3), round(max(ts), 3)]
            row["host_fill_ms"] = round(1e3 * best, 1)
            same = torch.equal(filled[mask], texture.fill(normal, mask, 32)[mask])
            row["host_fill_keeps_the_mask_texels_like_the_device"] = bool(same)
            if F <= 5000:
                info = {}
                ref.rasterize(v_clip.cpu().numpy(), at.ft.cpu().numpy(), res, res, info)
                covered, exact = int(info["covered"].sum()), True
                row["faces_on_the_second_path"] = len(info["large"])
            else:
                covered, exact = hit, False
            row["atomic_min_samples"], row["atomic_min_samples_exact"] = covered, exact
            row["atomic_min_gb_per_s_over_whole_call"] = round(8 * covered / row["rasterize_ms"] / 1e6, 3)
            tc64, tr = torch_grid_put(size, size, coords, values, valid, mr), (cur, cur_cnt)
            row["grid_put_max_abs_difference_to_torch"] = float((tc64[0] - tr[0]).abs().max())
            row["grid_put_holes_equal_to_torch"] = bool(torch.equal(tc64[1] == 0, tr[1] == 0))
            row["bake_albedo_range"] = [float(baked.albedo.min()), float(baked.albedo.max())]
            rows.append(row)
            print(json.dumps(row), flush=True)
    return {
        "what": "texture bake: csrc/texture.hip against the reference's stages restated in torch on the same device (grid put) and "
                "its scipy + sklearn tail on the host (fill); tools/texture_time.py",
        "device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "iters_per_window": args.iters, "host_runs": args.host_runs,
        "statistic": "device and torch: median (and min, max) over the rounds of a window's time per call by device events, stages "
                     "alternating inside a round, one warm-up round (bake: windows of one call); host: wall clock, best of host_runs",
        "atomic_rate_note": "atomic_min_gb_per_s_over_whole_call divides by the whole rasterize call, not by pass 1 alone; the chip-wide "
                            "rate known for atomics on this part, about 1.3 TB/s of added bytes, is for 32-bit float adds: no rate for a "
                            "64-bit integer min was measured, so the comparison rests on an unmeasured number",
        "rows": rows,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--host-runs", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/texture_time.py needs a ROCm device: a time taken anywhere else says nothing")
    doc = measure(args, torch.device("cuda:0"))
    print(json.dumps(doc, indent=1), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
