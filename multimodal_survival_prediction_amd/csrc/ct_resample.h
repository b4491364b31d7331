// The one arithmetic of both CT routes (preproc.hip: float volumes, ct_ingest.hip: the stored types of NIfTI files): min-max
// normalisation + scipy.ndimage.zoom(order=1, grid_mode=False) of one output voxel.
//
// Output index o maps to input coordinate o * (in - 1) / (out - 1) in fp64 (0 when out == 1); linear interpolation between the two
// neighbours per axis.  In exact arithmetic the normalisation (x - min) / (max - min + 1e-8) is affine and commutes with the
// interpolation; in fp32 it does not -- a (1 - f) + a f is not a -- so the reference value is subtracted FIRST: the eight
// neighbours enter as t = x - min >= 0 (exact for the integer types of a CT), the weights are in [0, 1], hence
//   * a constant volume is 0 exactly and no output is below 0,
//   * the rounding error scales with the volume's contrast, not with its offset.
// Contraction into FMAs is switched off inside these bodies: every instantiation rounds each product and each sum, so a volume gives
// the same bits whichever kernel it is inlined into.
#pragma once
#include "common.h"

// step of the input coordinate per output index along one axis
__device__ __forceinline__ double ct_axis_step(int in, int out) { return out > 1 ? (double)(in - 1) / (out - 1) : 0.0; }

// 1 / (max - min + 1e-8) for values slope * r + inter, as a factor on |slope| (r - min): a = |slope|
__device__ __forceinline__ float ct_norm_scale(float a, float rlo, float rhi) {
#pragma clang fp contract(off)
    return a / (a * (rhi - rlo) + 1e-8f);
}

// at(d, h, w) -> t of input voxel (d, h, w), already minus the reference value; in: the input grid; (od, oh, ow): the output voxel;
// (sd, sh, sw): ct_axis_step per axis.  Returns the interpolated t times sc.
template <class At>
__device__ __forceinline__ float ct_interp_norm(At at, Dims3 in, int od, int oh, int ow, double sd, double sh, double sw, float sc) {
#pragma clang fp contract(off)
    const double cd = od * sd, ch = oh * sh, cw = ow * sw;
    const int d0 = (int)cd, h0 = (int)ch, w0 = (int)cw;
    const int d1 = d0 + 1 < in.D ? d0 + 1 : d0, h1 = h0 + 1 < in.H ? h0 + 1 : h0, w1 = w0 + 1 < in.W ? w0 + 1 : w0;
    const float fd = (float)(cd - d0), fh = (float)(ch - h0), fw = (float)(cw - w0);
    const float c00 = at(d0, h0, w0) * (1 - fw) + at(d0, h0, w1) * fw, c01 = at(d0, h1, w0) * (1 - fw) + at(d0, h1, w1) * fw;
    const float c10 = at(d1, h0, w0) * (1 - fw) + at(d1, h0, w1) * fw, c11 = at(d1, h1, w0) * (1 - fw) + at(d1, h1, w1) * fw;
    const float v = (c00 * (1 - fh) + c01 * fh) * (1 - fd) + (c10 * (1 - fh) + c11 * fh) * fd;
    return v * sc;
}
