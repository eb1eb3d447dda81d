/*
 * TEST INFRASTRUCTURE ONLY (tests/filter_ref.py compiles it).
 *
 * Kernel-order restatement of resize -> crop -> hflip over tap tables passed
 * in: the order of operations of oracle/stbir_oracle.c orc_resize_crop_vfirst
 * (vertical pass first, in byte units, each sum an fmaf chain in tap order
 * starting from 0, then the horizontal pass the same way, then stbir's encode
 * (uint8)trunc(clamp(v + 0.5, 0, 255))), with the tables a caller's instead
 * of the oracle's own triangle ones.  With the product's tables
 * (mxd_axis_taps_filter) this is what the HIP kernels must give bit for bit,
 * for any filter: negative lobes overshoot and the encode's clamp bounds them.
 *
 * Tables: first[n], count[n] and weights[n][width] of every output of the
 * axis (n = resize size), zero padded.  Writes the crop window (cx, cy, cw,
 * ch), mirrored when flip, as ch x cw x c bytes.  Build with
 * -ffp-contract=off.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

int filter_vfirst(const uint8_t* src, int w, int h, int c, int64_t stride, uint8_t* dst, const int32_t* xfirst,
                  const int32_t* xcount, const float* xw, int xwidth, const int32_t* yfirst, const int32_t* ycount,
                  const float* yw, int ywidth, int cx, int cy, int cw, int ch, int flip) {
  if (w <= 0 || h <= 0 || c < 1 || c > 4 || cw <= 0 || ch <= 0 || cx < 0 || cy < 0) return -1;
  float* vrow = (float*)malloc(sizeof(float) * (size_t)w * c);
  if (!vrow) return -1;
  int xlo = xfirst[cx], xhi = xfirst[cx] + xcount[cx] - 1;
  for (int ox = cx; ox < cx + cw; ox++) {
    if (xfirst[ox] < xlo) xlo = xfirst[ox];
    if (xfirst[ox] + xcount[ox] - 1 > xhi) xhi = xfirst[ox] + xcount[ox] - 1;
  }
  if (xlo < 0 || xhi >= w) {
    free(vrow);
    return -2;
  }
  for (int r = 0; r < ch; r++) {
    const int oy = cy + r;
    const int a = yfirst[oy], n = ycount[oy];
    const float* cf = yw + (size_t)oy * ywidth;
    if (a < 0 || a + n > h) {
      free(vrow);
      return -2;
    }
    for (int i = xlo * c; i < (xhi + 1) * c; i++) {
      float v = 0.0f;
      for (int k = 0; k < n; k++) v = fmaf(cf[k], (float)src[(size_t)(a + k) * stride + i], v);
      vrow[i] = v;
    }
    uint8_t* d = dst + (size_t)r * cw * c;
    for (int x = 0; x < cw; x++) {
      const int ox = cx + (flip ? cw - 1 - x : x);
      const int xa = xfirst[ox], xn = xcount[ox];
      const float* cfx = xw + (size_t)ox * xwidth;
      for (int k2 = 0; k2 < c; k2++) {
        float hsum = 0.0f;
        for (int k = 0; k < xn; k++) hsum = fmaf(cfx[k], vrow[(xa + k) * c + k2], hsum);
        float f = hsum + 0.5f;
        if (f < 0.0f) f = 0.0f;
        if (f > 255.0f) f = 255.0f;
        d[x * c + k2] = (uint8_t)f;
      }
    }
  }
  free(vrow);
  return 0;
}
