"""Model compression (SPEC M21; 4.23): a k-means codebook for the 45 SH-rest coefficients with 16-bit indices, the
answer of Compact3D, LightGaussian, Niedermayr et al.'s "Compressed 3DGS" and gsplat's compression strategy, and a container that
keeps every other field of the PLY lossless.

    codebook, idx, history = kmeans(x, K, iters=10, weights=None, seed=0)        any [P,D] float32 tensor on the GPU, D <= 64
    save_compressed(model, path, sh_codes=4096, weights=contribution_scores(...).weight_sum)
    load_compressed(model, path)                                                 the attributes load_ply fills, dense again
    compressed_size_report(path)                                                 bytes per field

The two device steps are diff_gaussian_rasterization.vq_assign (nearest code on the f32 MFMA, no [P,K] matrix) and vq_update
(centroids in double, in a fixed order, without atomics), so one compression of one model writes the same file on every run.
Opacity, scales and the pixel-size thresholds decide the multi-scale filters at exact ties (SPEC M1-M4): they are stored as they
are, never rounded.  Not here: rendering from indices, quantisation-aware fine-tuning, entropy coding, half precision, codebooks
for other attributes (the kernels take any D <= VQ_MAX_DIM)."""
import os
import zipfile

import numpy as np
import torch
import torch.nn as nn
from diff_gaussian_rasterization import VQ_MAX_CODES, VQ_MAX_DIM, vq_assign, vq_update

FORMAT_VERSION = 1
# name in the file -> (attribute, shape after the row count); float32 unless said otherwise
_LOSSLESS = (("xyz", "_xyz"), ("opacity", "_opacity"), ("scaling", "_scaling"), ("rotation", "_rotation"),
             ("occ_multiplier", "_occ_multiplier"), ("dc_delta", "_dc_delta"), ("max_pixel_sizes", "max_pixel_sizes"),
             ("min_pixel_sizes", "min_pixel_sizes"))


def kmeans(x, K, iters=10, tol=0.0, weights=None, seed=0, init=None):
    """(codebook [K,D] float32, idx [P] int32, history: the weighted distortion sum w_i err_i of every assignment, the final one
    last).  Initialised from K distinct rows drawn by a seeded CPU generator permutation (or from `init` [K,D]); per iteration
    assign, update, reseed — the e-th code without members, in ascending k, takes the row of the e-th largest w_i err_i (stable
    descending sort) — and one host read, of the distortion and the number of empty codes.  Stops after `iters` iterations or when
    the distortion fell by less than `tol` of itself; a final assignment makes idx belong to the returned codebook."""
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError("kmeans: x must be a tensor [P,D]")
    P, D = (int(n) for n in x.shape)
    K, iters = int(K), int(iters)
    if not 1 <= D <= VQ_MAX_DIM:
        raise ValueError(f"kmeans: D = {D}, 1 .. {VQ_MAX_DIM} columns are supported")
    if not 1 <= K <= VQ_MAX_CODES:
        raise ValueError(f"kmeans: K = {K}, 1 .. {VQ_MAX_CODES} codes are supported")
    if K > P:
        raise ValueError(f"kmeans: K = {K} codes for P = {P} rows; a codebook cannot be larger than the data")
    if iters < 0:
        raise ValueError("kmeans: iters must not be negative")
    if weights is not None and (not torch.is_tensor(weights) or tuple(weights.shape) != (P,)):
        raise ValueError(f"kmeans: weights must be a tensor [{P}]")
    if init is None:
        rows = torch.randperm(P, generator=torch.Generator().manual_seed(int(seed)))[:K]
        codebook = x.detach()[rows.to(x.device)].contiguous()
    else:
        if tuple(init.shape) != (K, D):
            raise ValueError(f"kmeans: init must be [{K},{D}], got {tuple(init.shape)}")
        codebook = init.detach().to(x.device).contiguous()
    w64 = None if weights is None else weights.double()
    history = []
    for _ in range(iters):
        idx, err = vq_assign(x, codebook)
        score = err.double() if w64 is None else err.double() * w64
        new, _, count = vq_update(x, idx, codebook, weights)
        empty = count == 0
        distortion, n_empty = torch.stack((score.sum(), empty.sum().double())).tolist()           # the iteration's host read
        if n_empty:
            worst = torch.sort(score, descending=True, stable=True).indices[:K]
            rank = (torch.cumsum(empty, 0) - 1).clamp_(min=0)
            new = torch.where(empty[:, None], x[worst[rank]], new)
        codebook = new
        history.append(distortion)
        if len(history) > 1 and history[-2] - distortion < tol * history[-2]:
            break
    idx, err = vq_assign(x, codebook)
    history.append(float((err.double() if w64 is None else err.double() * w64).sum()))
    return codebook, idx, history


def _np(t):
    return t.detach().cpu().numpy()


def sh_rows(model):
    """[P, 3 n] float32: _features_rest in the PLY's channel-major flattening, so the file and the PLY agree on what a row is"""
    return model._features_rest.detach().transpose(1, 2).flatten(start_dim=1).contiguous()


def save_compressed(model, path, sh_codes=4096, iters=10, weights=None, seed=0, tol=0.0, quantised=None):
    """One .npz (numpy.savez_compressed): _features_rest as a k-means codebook [K,D] float32 (K = min(sh_codes, P)) and indices —
    uint16 when K <= 65536, else int32 — and every other field save_ply writes, bit for bit.  `weights` [P] >= 0: a per-Gaussian
    sensitivity, e.g. contribution_scores(...).weight_sum.  `quantised` = (codebook [K,D], idx [P]) stores a quantisation made
    elsewhere instead of running k-means (which needs the model on the GPU).  Returns (codebook, idx)."""
    rows = sh_rows(model)
    P, D = (int(n) for n in rows.shape)
    if quantised is None:
        if D == 0 or P == 0:
            codebook, idx = rows.new_zeros((0, D)), torch.zeros(P, dtype=torch.int32)
        else:
            codebook, idx, _ = kmeans(rows, min(int(sh_codes), P), iters=iters, tol=tol, weights=weights, seed=seed)
    else:
        codebook, idx = quantised
    cb = np.ascontiguousarray(_np(codebook), dtype=np.float32).reshape(len(codebook), D)
    ix = _np(idx).astype(np.int64).reshape(-1)
    if len(ix) != P or (P and (ix.min() < 0 or ix.max() >= max(len(cb), 1))):
        raise ValueError(f"save_compressed: {len(ix)} indices into {len(cb)} codes for {P} Gaussians")
    fields = {"format_version": np.int32(FORMAT_VERSION), "sh_degree": np.int32(model.max_sh_degree),
              "sh_codebook": cb, "sh_index": ix.astype(np.uint16 if len(cb) <= 65536 else np.int32),
              "f_dc": _np(model._features_dc.detach().transpose(1, 2).flatten(start_dim=1)).astype(np.float32),
              "base_gaussian_mask": _np(model.base_gaussian_mask).astype(np.bool_)}
    for name, attr in _LOSSLESS:
        fields[name] = np.ascontiguousarray(_np(getattr(model, attr)), dtype=np.float32)
    if getattr(model, "filter_3D", None) is not None:
        fields["filter_3D"] = _np(model.filter_3D).reshape(P).astype(np.float32)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:                                    # a file object: savez does not append ".npz" to the name
        np.savez_compressed(f, **fields)
    return codebook, idx


def load_compressed(model, path, device="cuda", multi_occ=False, multi_dc=False):
    """fills the attributes load_ply fills; _features_rest = codebook[idx], every other field as it was saved"""
    with np.load(path) as z:
        v = {k: z[k] for k in z.files}
    if int(v["format_version"]) != FORMAT_VERSION:
        raise ValueError(f"{path}: format version {int(v['format_version'])}, this build reads {FORMAT_VERSION}")
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float, device=device)
    P = len(v["xyz"])
    cb, ix = v["sh_codebook"], v["sh_index"].astype(np.int64)
    D = cb.shape[1]
    rest = cb[ix] if P and D else np.zeros((P, D), np.float32)
    model._xyz = nn.Parameter(t(v["xyz"]).requires_grad_(True))
    model._features_dc = nn.Parameter(t(v["f_dc"].reshape(P, 3, -1)).transpose(1, 2).contiguous().requires_grad_(True))
    model._features_rest = nn.Parameter(t(rest.reshape(P, 3, D // 3)).transpose(1, 2).contiguous().requires_grad_(True))
    model._opacity = nn.Parameter(t(v["opacity"]).requires_grad_(True))
    model._occ_multiplier = nn.Parameter(t(v["occ_multiplier"]), requires_grad=multi_occ)
    model._dc_delta = nn.Parameter(t(v["dc_delta"]), requires_grad=multi_dc)
    model._scaling = nn.Parameter(t(v["scaling"]).requires_grad_(True))
    model._rotation = nn.Parameter(t(v["rotation"]).requires_grad_(True))
    model.base_gaussian_mask = torch.from_numpy(v["base_gaussian_mask"].astype(np.bool_)).to(device)
    model.max_pixel_sizes = t(v["max_pixel_sizes"])
    model.min_pixel_sizes = t(v["min_pixel_sizes"])
    if "filter_3D" in v:
        model.filter_3D = t(v["filter_3D"][:, None])
    model.active_sh_degree = model.max_sh_degree = int(v["sh_degree"])
    return model


def compressed_size_report(path):
    """{field: bytes it takes in the file (deflated data plus its zip records), "total": the file's size}; the fields add up to
    the total"""
    total = os.path.getsize(path)
    with zipfile.ZipFile(path) as z:
        infos = sorted(z.infolist(), key=lambda i: i.header_offset)
        ends = [i.header_offset for i in infos[1:]] + [z.start_dir]
        report = {}
        for i, end in zip(infos, ends):
            name = i.filename[:-4] if i.filename.endswith(".npy") else i.filename
            central = 46 + len(i.filename.encode()) + len(i.extra) + len(i.comment)
            report[name] = (end - i.header_offset) + central
        report["end_of_archive"] = total - z.start_dir - sum(46 + len(i.filename.encode()) + len(i.extra) + len(i.comment)
                                                               for i in infos)
    report["total"] = total
    return report
