// Index arithmetic of the folded pack layers' exact border (csrc/pack_border.hip), free of HIP so that the host tests compile it alone.
//
// The folded convolution evaluates conv3d on the zero-extended packed tensor everywhere, the reference zeroes conv3d's result T outside the
// H2 x W2 image.  conv3d reaches one pixel, so outside the image T depends on the data only on the RING at distance 1:
//     y_ref(p) = y_fold(p) - sum_{t : p+t on the ring} W[t] . U(p+t) - sum_{t : p+t outside} S[t],     U = T - b3 on the ring.
// Ring lines (edge e): 0 top row y' = -1, 1 bottom row y' = H2, both over x' = -1 .. W2 (corners included, position i = x' + 1);
//                      2 left column x' = -1, 3 right column x' = W2, both over y' = 0 .. H2-1 (position i = y').
// Border pixels: j = distance to the near edge < pad = k/2.  A pixel j away from an edge meets that edge's ring line with ONE tap row / column.
// Pixel classes per axis: 0 .. pad-1 = that far from the low edge, pad = interior, 2 pad - j = j away from the high edge (needs extent >= 2 pad).
#pragma once

#ifndef PB_HD
#ifdef __HIPCC__
#define PB_HD __host__ __device__ inline
#else
#define PB_HD inline
#endif
#endif

#define PB_CLASS_SPLITS 64     // partial sums per pixel class (mte_pack_border_class_sums)
#define PB_RING_BLOCKS 64      // workgroups per edge of the ring stencil's weight gradient

// ---- the ring stencil ------------------------------------------------------------------------------------------------------------------
PB_HD int pb_edge_len(int e, int H2, int W2) { return e < 2 ? W2 + 2 : H2; }
// packed-image pixel (h, w) that tap a = 0..2 along edge e reads at ring position i; false = outside the image (contributes nothing)
PB_HD bool pb_edge_src(int e, int i, int a, int H2, int W2, int* h, int* w) {
    if (e < 2) { *h = e == 0 ? 0 : H2 - 1; *w = i + a - 2; return *w >= 0 && *w < W2; }
    *w = e == 2 ? 0 : W2 - 1; *h = i + a - 1; return *h >= 0 && *h < H2;
}
// index into K3[4][3][3][3] = [f][kd][dh][dw]: across the edge only the tap that reaches back into the image counts
PB_HD int pb_k3_index(int e, int f, int kd, int a) {
    const int fix = (e == 0 || e == 2) ? 2 : 0;
    return e < 2 ? ((f * 3 + kd) * 3 + fix) * 3 + a : ((f * 3 + kd) * 3 + a) * 3 + fix;
}
// is pixel (h, w) on the source line of edge e?  If so, tap a of ring position i = *along + *off - a reads it (for the i that lie inside the edge's length)
PB_HD bool pb_edge_of_pixel(int e, int h, int w, int H2, int W2, int* along, int* off) {
    if (e < 2) { *along = w; *off = 2; return h == (e == 0 ? 0 : H2 - 1); }
    *along = h; *off = 1; return w == (e == 2 ? 0 : W2 - 1);
}

// ---- the border GEMMs --------------------------------------------------------------------------------------------------------------------
// tap row (column) with which a pixel j away from the near (far = 0) / far (far = 1) edge meets that edge's ring line
PB_HD int pb_tap(int far, int j, int pad) { return far ? pad + 1 + j : pad - 1 - j; }
// GEMM column of (far, j, co): the edges and distances are stacked in the output-channel dimension
PB_HD int pb_col(int far, int j, int co, int pad, int Co) { return (far * pad + j) * Co + co; }
// the (far, j) whose tap is t; false for the centre tap, which never leaves the image
PB_HD bool pb_tap_owner(int t, int pad, int* far, int* j) {
    if (t == pad) return false;
    *far = t > pad; *j = t > pad ? t - pad - 1 : pad - 1 - t;
    return true;
}
PB_HD int pb_class(int r, int n, int pad) { return r < pad ? r : (n - 1 - r < pad ? 2 * pad - (n - 1 - r) : pad); }
PB_HD bool pb_tap_outside(int cls, int t, int pad) { return cls < pad ? t < pad - cls : (cls > pad ? t > 3 * pad - cls : false); }
PB_HD int pb_class_count(int cls, int n, int pad) { return cls == pad ? n - 2 * pad : 1; }     // pixels of a class along one axis
PB_HD int pb_class_first(int cls, int n, int pad) { return cls < pad ? cls : (cls == pad ? pad : n - 1 - (2 * pad - cls)); }

// border pixels in a fixed order: pad top rows, pad bottom rows, then the left and right columns between them
PB_HD long pb_border_count(int H2, int W2, int pad) { return 2L * pad * W2 + 2L * pad * (H2 - 2 * pad); }
PB_HD void pb_border_pixel(long idx, int H2, int W2, int pad, int* r, int* x) {
    const long rows = 2L * pad * W2;
    if (idx < rows) { const int q = (int)(idx / W2); *x = (int)(idx % W2); *r = q < pad ? q : H2 - 2 * pad + q; return; }
    idx -= rows;
    const int q = (int)(idx % (2 * pad));
    *r = pad + (int)(idx / (2 * pad)); *x = q < pad ? q : W2 - 2 * pad + q;
}
PB_HD bool pb_shape_ok(int H2, int W2, int k) { return (k & 1) && k >= 3 && H2 >= 2 * (k / 2) && W2 >= 2 * (k / 2); }
