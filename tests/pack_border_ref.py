"""fp64 references of csrc/pack_border.hip: the exact border of a folded pack layer from the one-pixel ring (include/mte_kernels.h).

Layouts follow the kernels (channels last): P [B,H2,W2,D] packed tensor, K3 [4,3,3,3], b3 [4], W [Co,4D,k,k]; ring lines Rr [2B,W2+2,4D] (top, bottom;
position i = x'+1) and Rc [2B,H2,4D] (left, right); GEMM columns (far, j, co) -> (far*pad + j)*Co + co.  The forward pieces are differentiable torch
code, so autograd on their composition gives every gradient; the backward kernels have explicit references that the CPU test checks against it."""
import torch
import torch.nn.functional as F


# ---- index arithmetic (csrc/pack_border_plan.hpp) -----------------------------------------------------------------------------------------
def tap(far, j, pad):
    return pad + 1 + j if far else pad - 1 - j


def classes_of(r, n, pad):
    """classes of position r along an axis of n pixels: [] interior; two entries only where n < 2 pad"""
    out = []
    if r < pad:
        out.append(r)
    if n - 1 - r < pad:
        out.append(2 * pad - (n - 1 - r))
    return out


def class_of(r, n, pad):
    assert n >= 2 * pad
    c = classes_of(r, n, pad)
    return c[0] if c else pad


def tap_outside(cls, t, pad):
    return t < pad - cls if cls < pad else (t > 3 * pad - cls if cls > pad else False)


def k3_fixed(e):
    return 2 if e in (0, 2) else 0


# ---- the two formulations of the layer -------------------------------------------------------------------------------------------------------
def conv3d_on(P, K3, b3, ext):
    """conv3d(1->4) of the zero-extended packed tensor on the image grown by `ext` pixels: [B, 4D, H2+2ext, W2+2ext] (channel f*D+d)"""
    B, H2, W2, D = P.shape
    v = P.permute(0, 3, 1, 2).unsqueeze(1)                           # [B,1,D,H2,W2]
    v = F.pad(v, (ext, ext, ext, ext))
    T = F.conv3d(v, K3.unsqueeze(1), b3, padding=1)                  # padding 1 in (d, h, w): the grown grid keeps its size
    return T.reshape(B, 4 * D, H2 + 2 * ext, W2 + 2 * ext)


def layer_reference(P, K3, b3, W, b):
    """conv2d(zero_pad(conv3d(P))) + b -> [B,H2,W2,Co]: the reference chain (layers01.py:241-247)"""
    k = W.shape[-1]
    return F.conv2d(conv3d_on(P, K3, b3, 0), W, b, padding=k // 2).permute(0, 2, 3, 1)


def layer_folded(P, K3, b3, W, b):
    """what the folded convolution computes: conv_k over conv3d of the zero-extended tensor, evaluated outside the image too"""
    k = W.shape[-1]
    return F.conv2d(conv3d_on(P, K3, b3, k // 2), W, b).permute(0, 2, 3, 1)


# ---- ring stencil ---------------------------------------------------------------------------------------------------------------------------------
def ring_fwd(P, K3):
    """(Rr, Rc): conv3d's data part on the ring, taken from the full conv3d on the image grown by one pixel"""
    B, H2, W2, D = P.shape
    U = conv3d_on(P, K3, torch.zeros(4, dtype=P.dtype), 1)           # [B,4D,H2+2,W2+2]
    Rr = torch.cat([U[:, :, 0, :], U[:, :, H2 + 1, :]], 0).permute(0, 2, 1)
    Rc = torch.cat([U[:, :, 1:H2 + 1, 0], U[:, :, 1:H2 + 1, W2 + 1]], 0).permute(0, 2, 1)
    return Rr.contiguous(), Rc.contiguous()


def _edge_line(P, e):
    """source line of edge e, zero-padded so that ring position i and tap a read index i + a: [B, len + 2, D + 2]"""
    B, H2, W2, D = P.shape
    line = P[:, 0 if e == 0 else H2 - 1] if e < 2 else P[:, :, 0 if e == 2 else W2 - 1]
    return F.pad(line, (1, 1, 2, 2) if e < 2 else (1, 1, 1, 1))


def _k3(K3, e, a):
    return K3[:, :, k3_fixed(e), a] if e < 2 else K3[:, :, a, k3_fixed(e)]           # [4 f, 3 kd]


def ring_fwd_taps(P, K3):
    """the same by the kernel's tap arithmetic (pb_edge_src / pb_k3_index)"""
    B, H2, W2, D = P.shape
    out = []
    for e in range(4):
        n = W2 + 2 if e < 2 else H2
        L = _edge_line(P, e)
        U = torch.zeros(B, n, 4, D, dtype=P.dtype)
        for a in range(3):
            for kd in range(3):
                U = U + _k3(K3, e, a)[:, kd].view(1, 1, 4, 1) * L[:, a:a + n, kd:kd + D].unsqueeze(2)
        out.append(U.reshape(B, n, 4 * D))
    return torch.cat(out[:2], 0), torch.cat(out[2:], 0)


def unshuffle(Pt):
    """x [B,2H2,2W2,C] <- P [B,H2,W2,4C], d = 4c + 2*sy + sx"""
    B, H2, W2, D = Pt.shape
    return Pt.view(B, H2, W2, D // 4, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * H2, 2 * W2, D // 4)


def ring_bwd_data(dRr, dRc, K3, shape):
    """gradient of the packed tensor [B,H2,W2,D] through the ring stencil (the kernel adds unshuffle() of it to dx)"""
    B, H2, W2, D = shape
    dP = torch.zeros(shape, dtype=dRr.dtype)
    for e in range(4):
        n = W2 + 2 if e < 2 else H2
        g = (dRr if e < 2 else dRc)[(e & 1) * B:(e & 1) * B + B].view(B, n, 4, D)
        L = torch.zeros(B, n + 2, D + 2, dtype=dRr.dtype)
        for a in range(3):
            for kd in range(3):
                L[:, a:a + n, kd:kd + D] += (_k3(K3, e, a)[:, kd].view(1, 1, 4, 1) * g).sum(2)
        L = L[:, 2:-2, 1:-1] if e < 2 else L[:, 1:-1, 1:-1]
        if e < 2:
            dP[:, 0 if e == 0 else H2 - 1] += L
        else:
            dP[:, :, 0 if e == 2 else W2 - 1] += L
    return dP


def ring_bwd_weight(dRr, dRc, P):
    B, H2, W2, D = P.shape
    dK3 = torch.zeros(4, 3, 3, 3, dtype=P.dtype)
    for e in range(4):
        n = W2 + 2 if e < 2 else H2
        g = (dRr if e < 2 else dRc)[(e & 1) * B:(e & 1) * B + B].view(B, n, 4, D)
        L = _edge_line(P, e)
        for a in range(3):
            for kd in range(3):
                s = (g * L[:, a:a + n, kd:kd + D].unsqueeze(2)).sum((0, 1, 3))           # [4 f]
                if e < 2:
                    dK3[:, kd, k3_fixed(e), a] += s
                else:
                    dK3[:, kd, a, k3_fixed(e)] += s
    return dK3


# ---- ring weights, class table -------------------------------------------------------------------------------------------------------------------
def tap_sums(W, b3):
    """S [Co,k,k] = sum_f b3[f] sum_d W[co][f*D+d][t]"""
    Co, CT, k, _ = W.shape
    return (W.view(Co, 4, CT // 4, k, k).sum(2) * b3.view(1, 4, 1, 1)).sum(1)


def outside_mask(k, dtype=torch.float64):
    """[(2 pad+1), (2 pad+1), k, k]: 1 where tap (ty, tx) of a pixel of class (cy, cx) lies outside the image"""
    pad, nc = k // 2, 2 * (k // 2) + 1
    m = torch.zeros(nc, nc, k, k, dtype=dtype)
    for cy in range(nc):
        for cx in range(nc):
            for ty in range(k):
                for tx in range(k):
                    m[cy, cx, ty, tx] = float(tap_outside(cy, ty, pad) or tap_outside(cx, tx, pad))
    return m


def border_weights(W, b3):
    """(Wr [2 pad Co,4D,1,k], Wc [2 pad Co,4D,k,1], Dt [(2 pad+1)^2, Co]), the weights negated"""
    Co, CT, k, _ = W.shape
    pad = k // 2
    Wr = torch.cat([-W[:, :, tap(far, j, pad), :].unsqueeze(2) for far in (0, 1) for j in range(pad)], 0)
    Wc = torch.cat([-W[:, :, :, tap(far, j, pad)].unsqueeze(3) for far in (0, 1) for j in range(pad)], 0)
    Dt = -torch.einsum("yxst,cst->yxc", outside_mask(k, W.dtype), tap_sums(W, b3)).reshape(-1, Co)
    return Wr, Wc, Dt


def ring_gemms(Rr, Rc, Wr, Wc):
    """(corr_rows [2B,W2+2,N], corr_cols [2B,H2,N]): the zero-padded 1 x k / k x 1 convolutions along the ring lines"""
    k = Wr.shape[-1]
    cr = F.conv2d(Rr.permute(0, 2, 1).unsqueeze(2), Wr, padding=(0, k // 2)).squeeze(2).permute(0, 2, 1)
    cc = F.conv2d(Rc.permute(0, 2, 1).unsqueeze(3), Wc, padding=(k // 2, 0)).squeeze(3).permute(0, 2, 1)
    return cr, cc


def pixel_bias(Dt, r, x, H2, W2, pad):
    """class-table term of pixel (r, x).  One class per axis where the image has >= 2 pad pixels; a pixel within pad of BOTH opposite edges (smaller images)
    combines its classes by inclusion-exclusion -- the tap rows outside at the top and at the bottom are disjoint sets"""
    nc = 2 * pad + 1
    D = Dt.view(nc, nc, -1)
    Cy, Cx = classes_of(r, H2, pad), classes_of(x, W2, pad)
    v = torch.zeros_like(D[0, 0])
    for cy in Cy:
        v = v + D[cy, pad]
    for cx in Cx:
        v = v + D[pad, cx]
    for cy in Cy:
        for cx in Cx:
            v = v + D[cy, cx] - D[cy, pad] - D[pad, cx]
    return v


def border_apply(y, cr, cc, Dt, k):
    """y [B,H2,W2,Co] + ring terms + class table on the border pixels"""
    B, H2, W2, Co = y.shape
    pad = k // 2
    out = y.clone()
    for j in range(pad):
        if j < H2:
            out[:, j] += cr[:B, 1:W2 + 1, j * Co:(j + 1) * Co]
            out[:, H2 - 1 - j] += cr[B:, 1:W2 + 1, (pad + j) * Co:(pad + j + 1) * Co]
        if j < W2:
            out[:, :, j] += cc[:B, :, j * Co:(j + 1) * Co]
            out[:, :, W2 - 1 - j] += cc[B:, :, (pad + j) * Co:(pad + j + 1) * Co]
    for r in range(H2):
        for x in range(W2):
            if classes_of(r, H2, pad) or classes_of(x, W2, pad):
                out[:, r, x] += pixel_bias(Dt, r, x, H2, W2, pad)
    return out


def layer_ring(P, K3, b3, W, b):
    """the folded result corrected by the ring: equals layer_reference"""
    k = W.shape[-1]
    Rr, Rc = ring_fwd(P, K3)
    Wr, Wc, Dt = border_weights(W, b3)
    cr, cc = ring_gemms(Rr, Rc, Wr, Wc)
    return border_apply(layer_folded(P, K3, b3, W, b), cr, cc, Dt, k)


# ---- backward pieces (images with >= 2 pad pixels per axis, as the kernels require) ------------------------------------------------------------------
def border_gather(dy, k):
    """(Gr [2B,W2+2,N], Gc [2B,H2,N], dD [(2 pad+1)^2, Co])"""
    B, H2, W2, Co = dy.shape
    pad, nc = k // 2, 2 * (k // 2) + 1
    N = 2 * pad * Co
    Gr = torch.zeros(2 * B, W2 + 2, N, dtype=dy.dtype)
    Gc = torch.zeros(2 * B, H2, N, dtype=dy.dtype)
    for j in range(pad):
        Gr[:B, 1:W2 + 1, j * Co:(j + 1) * Co] = dy[:, j]
        Gr[B:, 1:W2 + 1, (pad + j) * Co:(pad + j + 1) * Co] = dy[:, H2 - 1 - j]
        Gc[:B, :, j * Co:(j + 1) * Co] = dy[:, :, j]
        Gc[B:, :, (pad + j) * Co:(pad + j + 1) * Co] = dy[:, :, W2 - 1 - j]
    dD = torch.zeros(nc, nc, Co, dtype=dy.dtype)
    for r in range(H2):
        for x in range(W2):
            cy, cx = class_of(r, H2, pad), class_of(x, W2, pad)
            if (cy, cx) != (pad, pad):
                dD[cy, cx] += dy[:, r, x].sum(0)
    return Gr, Gc, dD.view(nc * nc, Co)


def border_scatter(dWr, dWc, dD, W, b3):
    """(dW [Co,4D,k,k], db3 [4]) from the gradients of the negated ring weights and of the class table"""
    Co, CT, k, _ = W.shape
    pad, nc = k // 2, 2 * (k // 2) + 1
    dW = torch.zeros_like(W)
    for far in (0, 1):
        for j in range(pad):
            blk = slice((far * pad + j) * Co, (far * pad + j + 1) * Co)
            dW[:, :, tap(far, j, pad), :] -= dWr[blk, :, 0, :]
            dW[:, :, :, tap(far, j, pad)] -= dWc[blk, :, :, 0]
    dS = -torch.einsum("yxst,yxc->cst", outside_mask(k, W.dtype), dD.view(nc, nc, Co))
    Wv = W.view(Co, 4, CT // 4, k, k)
    dW = dW + (b3.view(1, 4, 1, 1, 1) * dS.view(Co, 1, 1, k, k)).expand_as(Wv).reshape(W.shape)
    db3 = (dS.view(Co, 1, 1, k, k) * Wv).sum((0, 2, 3, 4))
    return dW, db3
