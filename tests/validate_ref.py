"""NumPy restatement of ppn_pckh_match (include/ppn.h) on the packed arrays: the same inputs, the same three outputs,
written with explicit loops over p and g and independently of evaluate.assign_gt_multi.  Every f32 step is a NumPy f32
scalar operation, so it is rounded on its own as the kernel's is."""
import numpy as np

J = 17
F = np.float32


def joint_points(kp_cell, bbox, score):
    """One person's rows (kp_cell i32[18], bbox f32[18,4], score f32[18]) -> (x f32[17], y f32[17], s f32[17])."""
    x, y, s = np.zeros(J, F), np.zeros(J, F), np.zeros(J, F)
    for j in range(J):
        if kp_cell[j + 1] >= 0:
            b = bbox[j + 1]
            x[j] = (F(b[1]) + F(b[3])) / F(2)
            y[j] = (F(b[0]) + F(b[2])) / F(2)
            s[j] = score[j + 1]
    return x, y, s


def match_mask(px, py, gxy, head, thresh):
    """17 match bits of one (person, ground-truth person) pair."""
    bits = np.zeros(J, bool)
    with np.errstate(all="ignore"):
        for j in range(J):
            dx, dy = F(gxy[j, 0]) - px[j], F(gxy[j, 1]) - py[j]
            xx, yy = F(dx * dx), F(dy * dy)
            d = F(np.sqrt(F(xx + yy))) / F(head)
            bits[j] = bool(F(d) <= F(thresh))                       # False for NaN and +inf
    return bits


def pckh_match(count, kp_cell, bbox, score, gt_xy, gt_head, gt_count, image_index, rec_score, rec_label, rec_count,
               dist_thresh=0.5):
    """Updates rec_score f32[N,M,17], rec_label u8[N,M,17], rec_count i32[N] in place and returns the flag word."""
    B, M = kp_cell.shape[:2]
    N, gmax = gt_head.shape
    flags = 0
    for b in range(B):
        n = int(image_index[b])
        if n == -1:
            continue
        if n < -1 or n >= N:
            flags |= 1
            continue
        G = int(gt_count[n])
        if G < 0 or G > gmax:
            flags |= 2
            continue
        P = min(max(int(count[b]), 0), M)
        rec_count[n] = P if G > 0 else 0
        if G == 0 or P == 0:
            continue
        best_g, best_cnt, best_bits, pts = [], [], [], []
        for p in range(P):
            x, y, s = joint_points(kp_cell[b, p], bbox[b, p], score[b, p])
            pts.append(s)
            bg, bc, bb = 0, -1, None
            for g in range(G):
                bits = match_mask(x, y, gt_xy[n, g], gt_head[n, g], dist_thresh)
                c = int(bits.sum())
                if c > bc:                                          # strictly greater: the first g of the largest count
                    bg, bc, bb = g, c, bits
            best_g.append(bg); best_cnt.append(bc); best_bits.append(bb)
        win_p, win_cnt = [-1] * G, [0] * G                          # per g the running winner, strictly greater only
        for p in range(P):
            g = best_g[p]
            if best_cnt[p] > win_cnt[g]:
                win_p[g], win_cnt[g] = p, best_cnt[p]
        for p in range(P):
            rec_score[n, p] = pts[p]
            rec_label[n, p] = best_bits[p].astype(np.uint8) if win_p[best_g[p]] == p else 0
    return flags
