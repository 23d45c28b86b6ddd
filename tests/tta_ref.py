"""NumPy restatement of flip-averaged inference (include/ppn.h, ppn_tta_merge / ppn_tta_stage) and the case generators of
tests/test_tta_cpu.py and tests/test_tta_gpu.py.  Test infrastructure only.

Heads are f32 [B, C, H, W] (or [C, H, W]) with C = 6K + E*sH*sW: groups resp, conf, x, y, w, h of K channels, then
e[E][sH][sW].  The tables below are the project skeleton's, written out (tests/test_tta_cpu.py holds tta.mirror_tables()
to them).
"""
from __future__ import annotations

import numpy as np

KP_MIRROR = [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 13, 14, 15, 16, 17]
EDGE_MIRROR = [0, 1, 5, 6, 7, 2, 3, 4, 8, 9, 11, 10, 13, 12, 15, 14, 16]
K, E = len(KP_MIRROR), len(EDGE_MIRROR)
HALF = np.float32(0.5)

# (B, H, W, sH, sW).  The first three are the issue's: an odd W (a self-mirrored column) with sH != sW, 35 cells and three
# images; an even W no vector divides, batch 1; the real geometry.  VECTOR: the smallest grid whose rows are whole 16-byte
# vectors (the kernel's float4 path).  GROUPS: 289 cells, more than the 256 cell vectors of one workgroup (two cell groups,
# the second partly filled).  WIDE: the float4 path with two cell groups (1152 cells; beyond what the decode takes, merge only).
ODD = (3, 5, 7, 5, 3)
EVEN = (1, 4, 6, 3, 5)
REAL = (2, 24, 24, 21, 21)
VECTOR = (2, 3, 8, 3, 2)
GROUPS = (1, 17, 17, 2, 2)
WIDE = (1, 32, 36, 1, 2)


def channels(sH, sW):
    return 6 * K + E * sH * sW


def mirror_head(h, kp_mirror=KP_MIRROR, edge_mirror=EDGE_MIRROR, sH=21, sW=21):
    """mirror(Bm) of include/ppn.h: the head of a mirrored frame mapped back to the frame."""
    h = np.asarray(h, np.float32)
    single = h.ndim == 3
    if single:
        h = h[None]
    k, e = len(kp_mirror), len(edge_mirror)
    B, C, H, W = h.shape
    assert C == 6 * k + e * sH * sW
    u = h[:, :6 * k].reshape(B, 6, k, H, W)[:, :, list(kp_mirror)][..., ::-1].copy()
    u[:, 2] = np.float32(1.0) - u[:, 2]
    limbs = h[:, 6 * k:].reshape(B, e, sH, sW, H, W)[:, list(edge_mirror)][:, :, :, ::-1][..., ::-1]
    out = np.concatenate([u.reshape(B, 6 * k, H, W), limbs.reshape(B, e * sH * sW, H, W)], 1)
    out = np.ascontiguousarray(out, np.float32)
    return out[0] if single else out


def keys_of(head, sH, sW, k=K, e=E):
    """u64 [B,E,H,W]: float_bits(max_s) << 32 | ~s_first, s_first the lowest s of the maximum."""
    B, C, H, W = head.shape
    win = head[:, 6 * k:].reshape(B, e, sH * sW, H, W)
    s_first = np.argmax(win, axis=2)                                    # first maximum
    mx = np.take_along_axis(win, s_first[:, :, None], 2)[:, :, 0]
    bits = np.ascontiguousarray(mx, np.float32).view(np.uint32).astype(np.uint64)
    return (bits << np.uint64(32)) | (~s_first.astype(np.uint32)).astype(np.uint64)


def merge_ref(a, b, sH=21, sW=21, kp_mirror=KP_MIRROR, edge_mirror=EDGE_MIRROR):
    """(unary f32 [B,6K,H,W], keys u64 [B,E,H,W], head f32 [B,C,H,W]) of A = a and Bm = b."""
    a = np.asarray(a, np.float32)
    m = mirror_head(b, kp_mirror, edge_mirror, sH, sW)
    head = ((a + m) * HALF).astype(np.float32)
    k, e = len(kp_mirror), len(edge_mirror)
    return np.ascontiguousarray(head[:, :6 * k]), keys_of(head, sH, sW, k, e), head


def stage_ref(x, axis):
    return np.concatenate([x, np.flip(x, axis)], 0)


def dyadic_pair(seed, shape):
    """Heads A, Bm from {0, 1/8, .., 1}: every average is exact and window maxima are attained at several s."""
    B, H, W, sH, sW = shape
    rng = np.random.default_rng(seed)
    a, b = (rng.integers(0, 9, size=(B, channels(sH, sW), H, W)).astype(np.float32) / np.float32(8) for _ in range(2))
    return a, b


SUBNORMALS = np.array([0.0, 1e-44, 3e-39, 1.4e-45, 1.1754942e-38], np.float32)


def uniform_pair(seed, shape):
    """Heads A, Bm uniform in [0, 1); at one cell per image every channel of A, and of Bm at the mirrored cell, holds 0 or a
    subnormal (1e-44, 3e-39, ..): that cell's merged windows have subnormal maxima, and a sum of two subnormals halved."""
    B, H, W, sH, sW = shape
    rng = np.random.default_rng(seed)
    C = channels(sH, sW)
    a, b = (rng.random(size=(B, C, H, W), dtype=np.float32) for _ in range(2))
    for img in range(B):
        i, j = int(rng.integers(H)), int(rng.integers(W))
        a[img, :, i, j] = SUBNORMALS[rng.integers(0, len(SUBNORMALS), size=C)]
        b[img, :, i, W - 1 - j] = SUBNORMALS[rng.integers(0, len(SUBNORMALS), size=C)]
    return a, b


def backwards_argmax(a, b, sH, sW):
    """What a kernel would report that arg-maxes each window in Bm's OWN order (first maximum over s' = (ly, sW-1-lx)) and
    maps the index back: among ties in one window row it takes the LARGEST lx.  The ties test asserts the cases tell it
    apart from the specified first maximum in merged order."""
    head = merge_ref(a, b, sH, sW)[2]
    B, C, H, W = head.shape
    win = head[:, 6 * K:].reshape(B, E, sH, sW, H, W)[:, :, :, ::-1].reshape(B, E, sH * sW, H, W)
    sp = np.argmax(win, axis=2)
    return (sp // sW) * sW + (sW - 1 - sp % sW)


# ---- planted people (the default 384 x 384 / 24 x 24 / 21 x 21 geometry) ------------------------------------------------
def planted(people):
    """A perfect head built from the target encoder, as tests/test_oracle.py::test_target_encoder_roundtrip builds it."""
    from oracle import targets_ref as T
    tg = T.encode_targets(people)
    return np.concatenate([tg["delta"], np.ones_like(tg["delta"]), tg["tx"], tg["ty"], tg["tw"], tg["th"],
                           tg["te"].reshape(E * 441, 24, 24)], 0).astype(np.float32)


def mirror_person(p, inW=384, kp_mirror=KP_MIRROR):
    """x -> inW - x for the box centre and every point; points and `visible` permuted by kp_mirror (keypoint k is
    points[k - 1])."""
    cx, cy, w, h = p["bbox"]
    pts = np.asarray(p["points"], np.float32)
    vis = np.asarray(p["visible"])
    src = [kp_mirror[k] - 1 for k in range(1, len(kp_mirror))]
    new = pts[src].copy()
    new[:, 0] = np.float32(inW) - new[:, 0]
    return dict(bbox=(np.float32(inW) - np.float32(cx), cy, w, h), points=new, visible=vis[src].copy(), size=p["size"])


def people_in_distinct_cells(seed=5):
    """Three fully visible people whose keypoints of one kind never share a cell, every point at x = 16 c + f with an integer
    f in 1..15 (so that 1 - (16 - f) / 16 == f / 16 exactly) and every limb within the 21 x 21 window: 51 limb ones."""
    rng = np.random.default_rng(seed)
    people = []
    for ccx, ccy in ((6, 6), (12, 16), (17, 8)):
        def point(dx, dy):
            return np.array([16 * (ccx + dx) + int(rng.integers(1, 16)), 16 * (ccy + dy) + int(rng.integers(1, 16))],
                            np.float32)
        root = point(0, 0)
        pts = np.stack([point(int(rng.integers(-3, 4)), int(rng.integers(-3, 4))) for _ in range(K - 1)])
        people.append(dict(bbox=(root[0], root[1], np.float32(96), np.float32(128)), points=pts,
                           visible=np.ones(K - 1, bool), size=np.float32(16)))
    return people
