"""NumPy restatement of the train-time augmentation arithmetic (csrc/augment.hip, contract in include/ppn.h): f32 arrays,
the same operation order, the integer blend.  Written from the contract, not from the kernel and not from the reference;
tests/test_augment_cpu.py checks its properties and tests/test_augment_gpu.py compares the kernels with it bit for bit.

Every f32 product / sum below is ONE NumPy f32 operation (no fused multiply-add exists in NumPy), in the order the
contract writes them."""
import numpy as np

F32 = np.float32
MEAN = np.array([0.485, 0.456, 0.406], F32)
STD = np.array([0.229, 0.224, 0.225], F32)


def augment_images_ref(src, src_hw, inv, out_hw):
    """src u8[B,Hs,Ws,3], src_hw i[B,2] valid (h, w), inv f32[B,2,3] -> (u8 [B,outH,outW,3], f32 [B,3,outH,outW])."""
    src = np.asarray(src, np.uint8)
    inv = np.asarray(inv, F32)
    B, Hs, Ws, _ = src.shape
    outH, outW = out_hw
    ox = np.arange(outW, dtype=F32)[None, :]
    oy = np.arange(outH, dtype=F32)[:, None]
    out = np.zeros((B, outH, outW, 3), np.uint8)
    for b in range(B):
        h, w = int(src_hw[b][0]), int(src_hw[b][1])
        m = inv[b]
        sx = (m[0, 0] * ox + m[0, 1] * oy) + m[0, 2]
        sy = (m[1, 0] * ox + m[1, 1] * oy) + m[1, 2]
        assert sx.dtype == F32 and sy.dtype == F32
        flx, fly = np.floor(sx), np.floor(sy)
        a1 = np.rint((sx - flx) * F32(2048)).astype(np.int32)       # round half to even, like rintf
        b1 = np.rint((sy - fly) * F32(2048)).astype(np.int32)
        a0, b0 = 2048 - a1, 2048 - b1
        # indices far outside hit no tap whatever their value: clamp before the integer conversion
        ix = np.clip(flx, -2, Ws).astype(np.int32)
        iy = np.clip(fly, -2, Hs).astype(np.int32)
        img = src[b].astype(np.int32)

        def tap(y, x):
            ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
            v = img[np.clip(y, 0, Hs - 1), np.clip(x, 0, Ws - 1)]
            return np.where(ok[..., None], v, 0)

        t0 = tap(iy, ix) * a0[..., None] + tap(iy, ix + 1) * a1[..., None]
        t1 = tap(iy + 1, ix) * a0[..., None] + tap(iy + 1, ix + 1) * a1[..., None]
        v = (b0[..., None] * t0 + b1[..., None] * t1 + (1 << 21)) >> 22
        assert v.dtype == np.int32 and v.min() >= 0 and v.max() <= 255
        out[b] = v.astype(np.uint8)
    x = (out.astype(F32) - MEAN) / STD                                # one f32 subtract, one f32 divide
    return out, np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def _map(f, x, y):
    return (f[0, 0] * x + f[0, 1] * y) + f[0, 2], (f[1, 0] * x + f[1, 1] * y) + f[1, 2]


def augment_people_ref(people, visible, count, fwd, out_hw):
    """Packed arrays (people f32[B,pmax,5+2(K-1)], visible i32[B,pmax], count i32[B]) through fwd f32[B,2,3]
    -> the same three arrays, transformed and compacted (stable), tails zeroed."""
    people = np.asarray(people, F32)
    visible = np.asarray(visible, np.int32)
    fwd = np.asarray(fwd, F32)
    B, pmax, row = people.shape
    nk = (row - 5) // 2
    outH, outW = F32(out_hw[0]), F32(out_hw[1])
    po, vo, co = np.zeros_like(people), np.zeros_like(visible), np.zeros(B, np.int32)
    for b in range(B):
        f = fwd[b]
        n = 0
        for p in range(min(max(int(count[b]), 0), pmax)):
            P = people[b, p]
            Q = np.zeros(row, F32)
            vis = int(visible[b, p]) & 0xFFFFFFFF
            for j in range(nk):
                x, y = P[5 + 2 * j], P[6 + 2 * j]
                nx, ny = F32(0), F32(0)
                if not (x == 0 and y == 0):
                    tx, ty = _map(f, x, y)
                    if 0 <= tx < outW and 0 <= ty < outH:
                        nx, ny = tx, ty
                Q[5 + 2 * j], Q[6 + 2 * j] = nx, ny
                if nx == 0 and ny == 0:
                    vis &= ~(1 << j)
            if not np.any(Q[5:] != 0):
                continue                                              # nobody left of this person
            hw_, hh_ = np.floor(P[2] / F32(2)), np.floor(P[3] / F32(2))
            x1, x2, y1, y2 = P[0] - hw_, P[0] + hw_, P[1] - hh_, P[1] + hh_
            cs = [_map(f, cx, cy) for cx, cy in ((x1, y1), (x2, y1), (x1, y2), (x2, y2))]
            xs, ys = np.array([c[0] for c in cs], F32), np.array([c[1] for c in cs], F32)
            lx, ux = np.clip(xs.min(), F32(0), outW), np.clip(xs.max(), F32(0), outW)
            ly, uy = np.clip(ys.min(), F32(0), outH), np.clip(ys.max(), F32(0), outH)
            Q[0], Q[1], Q[2], Q[3] = (lx + ux) / F32(2), (ly + uy) / F32(2), ux - lx, uy - ly
            Q[4] = P[4]
            po[b, n] = Q
            vo[b, n] = np.array(vis & 0xFFFFFFFF, np.uint32).astype(np.int32)
            n += 1
        co[b] = n
    return po, vo, co


def unpack_people(people, visible, count):
    """The packed arrays back to the person lists targets.pack_people takes."""
    out = []
    for b in range(people.shape[0]):
        lst = []
        for p in range(int(count[b])):
            P = people[b, p]
            nk = (len(P) - 5) // 2
            lst.append(dict(bbox=tuple(P[0:4]), size=P[4], points=P[5:].reshape(nk, 2).copy(),
                            visible=[bool((int(visible[b, p]) >> k) & 1) for k in range(nk)]))
        out.append(lst)
    return out
