"""Writes ref_codebook_init_pins.npz: the reference's code-book initialisation (train.py:78-84) on four small seeded APE
maps.  The reference's own kmeans (train.py:36-56) is executed from its AST, as make_golden.py:kmeans_pins does (the
module itself imports the CUDA extensions); around it the train.py:80-83 expression is restated on the CPU:

    tot = torch.cat([kmeans(m.permute(1, 2, 0).reshape(-1, D).unique(dim=0), 80) for m in maps], 0)
    lut = kmeans(tot, tab_len).float()

Each map is [64, 48, 64] (a 64-d feature keeps the file small: tot and the LUT are [320, D] and [300, D] fp32),
piecewise constant over 4x4-pixel blocks drawn from 110 segment embeddings, so equal rows sit far apart in pixel order;
segment 0 is all zeros (unlabelled pixels), and two segments differ only by the sign of a zero (+0 / -0), which
unique(dim=0) merges.  The embeddings are multiples of 1/32 in [-4, 4], exact in float16, and are stored that way.
Stored: each map's embeddings and block labels, each view's unique rows as segment indices (the lowest segment with
that row's value), tot, the LUT and the CPU generator's state afterwards.  load_views() rebuilds maps and unique rows.

    python tests/golden/make_codebook_golden.py  (needs the reference checkout; set GOI_REFERENCE to its path)"""
import ast
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("GOI_REFERENCE", "/root/reference")


def reference_kmeans():
    src = open(os.path.join(REF, "train.py")).read()
    fn = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "kmeans")
    ns = {"torch": torch}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "train.py:kmeans", "exec"), ns)
    return ns["kmeans"]


def make_map(seed, D=64, H=48, W=64, segments=110):
    g = torch.Generator().manual_seed(seed)
    emb = torch.randint(-128, 129, (segments, D), generator=g).float() / 32
    emb[0] = 0.0  # unlabelled pixels
    emb[2] = emb[1]
    emb[1, 5] = 0.0
    emb[2, 5] = -0.0  # segments 1 and 2 are one row to unique(dim=0)
    labels = torch.randint(0, segments, (H // 4, W // 4), generator=g)
    labels[0, 0], labels[0, 1], labels[-1, -1], labels[-1, -2] = 0, 1, 2, 0
    return emb, labels


def expand(emb, labels):
    """the [D, H, W] map of 4x4-pixel blocks (tests rebuild the maps from the stored embeddings and block labels)"""
    lab = torch.as_tensor(labels).long().repeat_interleave(4, 0).repeat_interleave(4, 1)
    return torch.as_tensor(emb).float()[lab].permute(2, 0, 1).contiguous()


def load_views(z):
    """[(map [D, H, W] fp32, unique rows [N, D] fp32)] of the stored views"""
    out = []
    for v in range(int(z["n_views"])):
        emb = torch.from_numpy(z[f"emb{v}"]).float()
        out.append((expand(emb, z[f"labels{v}"]), emb[torch.from_numpy(z[f"unique_ids{v}"]).long()]))
    return out


def segment_ids(emb, rows):
    """index of the lowest segment whose embedding equals each row by value (-0 == 0)"""
    eq = (rows[:, None, :] == emb[None, :, :]).all(-1)
    assert bool(eq.any(1).all())
    return eq.float().argmax(1)


def main():
    kmeans = reference_kmeans()
    seed, per_view, tab_len = 2024, 80, 300
    segs = [make_map(100 + v) for v in range(4)]
    maps = [expand(*s) for s in segs]
    out = {"n_views": len(maps), "seed": seed, "per_view": per_view, "tab_len": tab_len}
    torch.manual_seed(seed)
    parts = []
    for v, m in enumerate(maps):
        u = m.permute(1, 2, 0).reshape(-1, m.shape[0]).unique(dim=0)
        emb = segs[v][0]
        assert torch.equal(emb.half().float(), emb)
        out[f"emb{v}"], out[f"labels{v}"] = emb.half().numpy(), segs[v][1].numpy().astype(np.int16)
        out[f"unique_ids{v}"] = segment_ids(emb, u).numpy().astype(np.int16)
        parts.append(kmeans(u.clone(), per_view))
    tot = torch.cat(parts, 0)
    out["tot"] = tot.numpy()
    out["lut"] = kmeans(tot.clone(), tab_len).float().numpy()
    out["rng_state"] = torch.get_rng_state().numpy()
    np.savez_compressed(os.path.join(HERE, "ref_codebook_init_pins.npz"), **out)
    print("wrote ref_codebook_init_pins", [out[f"unique_ids{v}"].shape[0] for v in range(len(maps))],
          "NaN LUT rows:", int(np.isnan(out["lut"]).any(1).sum()))


if __name__ == "__main__":
    main()
