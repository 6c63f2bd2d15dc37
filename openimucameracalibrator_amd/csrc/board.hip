// Radon marker checkerboard detection (applications/extract_board_to_json.cc, core::BoardExtractor::ExtractBoard of the
// reference for BoardType::RADON, which calls cv::findChessboardCornersSB with CALIB_CB_MARKER).  Our own detector
// after Duda & Frese (2018), specified by tests/board_restatement.py and DESIGN.md ("Board extraction"):
//   board_resize_gray_kernel   cv::resize (INTER_LINEAR, centre-aligned, 11-bit weights) then BGR2GRAY (14-bit weights)
//   board_response_kernel      3x3 binomial blur (integers x16), line sums over 2r+1 pixels along 0/45/90/135 degrees,
//                              ((max - min) / (16*255*(2r+1)))^2, polarity = brightest line; frame maximum
//   board_candidates_kernel    threshold * frame maximum, strict (2r+1)^2 non-maximum suppression, wave-ballot compaction
//   board_subpix_kernel        cornerSubPix's saddle iteration, one wave per candidate
//   (host)                     grid assembly: seed quad, homography growth, polarity alternation, W x H
//   board_marker_kernel        disc vs ring of every square of every assembled grid through the square's homography
//   (host)                     the three dots -> axes -> ids i*W + j
// The integer stages and the float32 response are exact, so they equal the restatement bit for bit; the sub-pixel
// sums are double and differ only in summation order.  No FMA contraction in this unit.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <set>
#include <vector>
#include "../../include/oicc_hip.h"
#include "frame_batches.h"
#include "hip_resources.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileX = 64, kTileY = 16;
constexpr int kMaxRadius = 8;
constexpr int kHalo = kMaxRadius + 1;
__constant__ int kDirX[4] = {1, 1, 0, -1};
__constant__ int kDirY[4] = {0, 1, 1, 1};

struct Cand { int32_t x, y; float resp; int32_t pol; };

// ---- 1: resize + gray ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void board_resize_gray_kernel(const uint8_t* __restrict__ src, int w, int h, int ch, int wd, int hd,
                                                                      const int* __restrict__ xi, const int* __restrict__ xw,
                                                                      const int* __restrict__ yi, const int* __restrict__ yw,
                                                                      uint8_t* __restrict__ gray) {
  const int x = blockIdx.x * kThreads + threadIdx.x, y = blockIdx.y, f = blockIdx.z;
  if (x >= wd) return;
  const int x0 = xi[x], x1 = min(x0 + 1, w - 1), y0 = yi[y], y1 = min(y0 + 1, h - 1);
  const int64_t wx1 = xw[x], wx0 = 2048 - wx1, wy1 = yw[y], wy0 = 2048 - wy1;
  const uint8_t* s = src + int64_t(f) * h * w * ch;
  int64_t c[3] = {0, 0, 0};
  for (int k = 0; k < ch; ++k) {
    const int64_t top = s[(int64_t(y0) * w + x0) * ch + k] * wx0 + s[(int64_t(y0) * w + x1) * ch + k] * wx1;
    const int64_t bot = s[(int64_t(y1) * w + x0) * ch + k] * wx0 + s[(int64_t(y1) * w + x1) * ch + k] * wx1;
    c[k] = (top * wy0 + bot * wy1 + (int64_t(1) << 21)) >> 22;
  }
  const int64_t g = ch == 1 ? c[0] : (1868 * c[0] + 9617 * c[1] + 4899 * c[2] + 8192) >> 14;
  gray[(int64_t(f) * hd + y) * wd + x] = uint8_t(g);
}

// ---- 2: blur + response ----------------------------------------------------------------------------------------------
// A 64 x 16 output tile: the gray tile with an (r+1) halo (clamped reads = replicated border), the horizontal blur, the
// vertical blur, then the line sums, all from LDS.
__global__ __launch_bounds__(kThreads) void board_response_kernel(const uint8_t* __restrict__ gray, int w, int h, int r, float inv,
                                                                   float* __restrict__ resp, uint8_t* __restrict__ pol,
                                                                   float* __restrict__ blurred, unsigned int* __restrict__ fmax) {
  constexpr int LX = kTileX + 2 * kHalo, LY = kTileY + 2 * kHalo;
  __shared__ int g[LY][LX];
  __shared__ int hb[LY][LX];
  __shared__ int B[LY][LX];
  const int f = blockIdx.z, tx0 = blockIdx.x * kTileX, ty0 = blockIdx.y * kTileY;
  const int R = r + 1, lx = kTileX + 2 * R, ly = kTileY + 2 * R;
  const uint8_t* G = gray + int64_t(f) * h * w;
  // staging: rows read as aligned 4-byte words (whole words inside the row when w % 4 == 0); the border words, and
  // every word of a row whose start is not 4-byte aligned, are read byte by byte with clamped (replicated) coordinates
  const int x_lo = tx0 - R, xa = x_lo >= 0 ? x_lo & ~3 : -((-x_lo + 3) & ~3), nwords = (tx0 + kTileX + R - xa + 3) / 4;
  const bool aligned = (w & 3) == 0;
  for (int k = threadIdx.x; k < nwords * ly; k += kThreads) {
    const int iy = k / nwords, X0 = xa + 4 * (k % nwords);
    const int Y = min(max(ty0 - R + iy, 0), h - 1);
    const uint8_t* row = G + int64_t(Y) * w;
    uint8_t v[4];
    if (aligned && X0 >= 0 && X0 + 3 < w) {
      const uint32_t word = *reinterpret_cast<const uint32_t*>(row + X0);
      for (int b = 0; b < 4; ++b) v[b] = uint8_t(word >> (8 * b));
    } else {
      for (int b = 0; b < 4; ++b) v[b] = row[min(max(X0 + b, 0), w - 1)];
    }
    for (int b = 0; b < 4; ++b) {
      const int ix = X0 + b - x_lo;
      if (ix >= 0 && ix < lx) g[iy][ix] = v[b];
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < lx * ly; k += kThreads) {
    const int iy = k / lx, ix = k % lx;
    hb[iy][ix] = (ix == 0 || ix == lx - 1) ? 0 : g[iy][ix - 1] + 2 * g[iy][ix] + g[iy][ix + 1];
  }
  __syncthreads();
  for (int k = threadIdx.x; k < lx * ly; k += kThreads) {
    const int iy = k / lx, ix = k % lx;
    B[iy][ix] = (iy == 0 || iy == ly - 1) ? 0 : hb[iy - 1][ix] + 2 * hb[iy][ix] + hb[iy + 1][ix];
  }
  __syncthreads();
  float local_max = 0.0f;
  for (int k = threadIdx.x; k < kTileX * kTileY; k += kThreads) {
    const int oy = k / kTileX, ox = k % kTileX, x = tx0 + ox, y = ty0 + oy;
    if (x >= w || y >= h) continue;
    const int cx = ox + R, cy = oy + R;
    const int64_t o = (int64_t(f) * h + y) * w + x;
    blurred[o] = float(B[cy][cx]) * 0.0625f;
    float v = 0.0f; int arg = 0;
    if (x >= r && x < w - r && y >= r && y < h - r) {
      int smax = -1, smin = 1 << 30;
      for (int d = 0; d < 4; ++d) {
        int s = 0;
        for (int t = -r; t <= r; ++t) s += B[cy + t * kDirY[d]][cx + t * kDirX[d]];
        if (s > smax) { smax = s; arg = d; }   // the first maximum, as numpy's argmax
        smin = min(smin, s);
      }
      const float dd = float(smax - smin) * inv;
      v = dd * dd;
    }
    resp[o] = v;
    pol[o] = uint8_t(arg);
    local_max = fmaxf(local_max, v);
  }
  for (int o = 32; o > 0; o >>= 1) local_max = fmaxf(local_max, __shfl_xor(local_max, o, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(fmax + f, __float_as_uint(local_max));   // non-negative floats order as uints
}

// ---- 3: candidates -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void board_candidates_kernel(const float* __restrict__ resp, const uint8_t* __restrict__ pol, int w, int h,
                                                                     int r, float threshold_rel, const unsigned int* __restrict__ fmax,
                                                                     int cap, int* __restrict__ count, Cand* __restrict__ cand) {
  const int x = blockIdx.x * kThreads + threadIdx.x, y = blockIdx.y, f = blockIdx.z;
  const float* Rf = resp + int64_t(f) * h * w;
  bool keep = false; float v = 0.0f;
  if (x < w) {
    v = Rf[int64_t(y) * w + x];
    keep = v > threshold_rel * __uint_as_float(fmax[f]);
    for (int dy = -r; dy <= r && keep; ++dy) {
      const int yy = y + dy;
      if (yy < 0 || yy >= h) continue;
      for (int dx = -r; dx <= r; ++dx) {
        const int xx = x + dx;
        if ((dx == 0 && dy == 0) || xx < 0 || xx >= w) continue;
        const float n = Rf[int64_t(yy) * w + xx];
        const bool later = dy > 0 || (dy == 0 && dx > 0);
        if (!(v > n || (v == n && later))) { keep = false; break; }
      }
    }
  }
  const unsigned long long m = __ballot(keep);
  if (m == 0) return;
  const int lane = threadIdx.x & 63;
  int base = 0;
  if (lane == 0) base = atomicAdd(count + f, __popcll(m));     // one vector atomic per wave
  base = __shfl(base, 0, 64);
  if (keep) {
    const int slot = base + __popcll(m & ((1ull << lane) - 1));
    if (slot < cap) cand[int64_t(f) * cap + slot] = Cand{x, y, v, int(pol[(int64_t(f) * h + y) * w + x])};
  }
}

// ---- 4: sub-pixel refinement ----------------------------------------------------------------------------------------
__device__ __forceinline__ double bilin(const float* I, int w, int h, double x, double y) {
  const double fx = floor(x), fy = floor(y), ax = x - fx, ay = y - fy;
  const int x0 = min(max(int(fx), 0), w - 1), x1 = min(max(int(fx) + 1, 0), w - 1);
  const int y0 = min(max(int(fy), 0), h - 1), y1 = min(max(int(fy) + 1, 0), h - 1);
  const double a = I[int64_t(y0) * w + x0], b = I[int64_t(y0) * w + x1], c = I[int64_t(y1) * w + x0], d = I[int64_t(y1) * w + x1];
  return (1 - ay) * ((1 - ax) * a + ax * b) + ay * ((1 - ax) * c + ax * d);
}

__device__ __forceinline__ double wsum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(kThreads) void board_subpix_kernel(const float* __restrict__ blurred, int w, int h, int F, int cap,
                                                                 const int* __restrict__ count, const Cand* __restrict__ cand, int win,
                                                                 int iterations, double eps, double* __restrict__ refined) {
  const int64_t wave = int64_t(blockIdx.x) * (kThreads / 64) + threadIdx.x / 64;
  if (wave >= int64_t(F) * cap) return;
  const int f = int(wave / cap), slot = int(wave % cap), lane = threadIdx.x & 63;
  if (slot >= min(count[f], cap)) return;
  const float* I = blurred + int64_t(f) * h * w;
  const Cand c = cand[wave];
  const double c0x = c.x, c0y = c.y;
  double cx = c0x, cy = c0y;
  const int side = 2 * win + 1;
  for (int it = 0; it < iterations; ++it) {
    double a = 0, b = 0, cc = 0, bb1 = 0, bb2 = 0;
    for (int k = lane; k < side * side; k += 64) {
      const double V = double(k / side - win), U = double(k % side - win);
      const double m = exp(-(U / win) * (U / win)) * exp(-(V / win) * (V / win));
      const double X = cx + U, Y = cy + V;
      const double gx = bilin(I, w, h, X + 1, Y) - bilin(I, w, h, X - 1, Y);
      const double gy = bilin(I, w, h, X, Y + 1) - bilin(I, w, h, X, Y - 1);
      const double gxx = gx * gx * m, gxy = gx * gy * m, gyy = gy * gy * m;
      a += gxx; b += gxy; cc += gyy; bb1 += gxx * U + gxy * V; bb2 += gxy * U + gyy * V;
    }
    a = wsum(a); b = wsum(b); cc = wsum(cc); bb1 = wsum(bb1); bb2 = wsum(bb2);
    const double det = a * cc - b * b;
    if (fabs(det) <= 2.220446049250313e-16 * 2.220446049250313e-16) break;
    const double s = 1.0 / det;
    const double nx = cx + cc * s * bb1 - b * s * bb2, ny = cy - b * s * bb1 + a * s * bb2;
    const double err = (nx - cx) * (nx - cx) + (ny - cy) * (ny - cy);
    cx = nx; cy = ny;
    if (cx < 0 || cx >= w || cy < 0 || cy >= h || err <= eps * eps) break;
  }
  if (fabs(cx - c0x) > win || fabs(cy - c0y) > win) { cx = c0x; cy = c0y; }
  if (lane == 0) { refined[2 * wave] = cx; refined[2 * wave + 1] = cy; }
}

// ---- 6: marker sampling ---------------------------------------------------------------------------------------------
struct GridRef { int32_t frame, A, B, corner0, cell0; };

__global__ __launch_bounds__(kThreads) void board_marker_kernel(const float* __restrict__ blurred, int w, int h, int num_grids,
                                                                 const GridRef* __restrict__ grids, const double* __restrict__ corners,
                                                                 int num_cells, double* __restrict__ disc, double* __restrict__ ring) {
  const int cell = blockIdx.x * kThreads + threadIdx.x;
  if (cell >= num_cells) return;
  int g = 0;
  while (g + 1 < num_grids && grids[g + 1].cell0 <= cell) ++g;
  const GridRef G = grids[g];
  const int k = cell - G.cell0, a = k / (G.B - 1), b = k % (G.B - 1);
  const double* C = corners + 2 * int64_t(G.corner0);
  auto P = [&](int i, int j, int c) { return C[2 * (i * G.B + j) + c]; };
  // Heckbert's unit square -> quad: (0,0),(1,0),(1,1),(0,1) -> (a,b),(a+1,b),(a+1,b+1),(a,b+1)
  const double x0 = P(a, b, 0), y0 = P(a, b, 1), x1 = P(a + 1, b, 0), y1 = P(a + 1, b, 1);
  const double x2 = P(a + 1, b + 1, 0), y2 = P(a + 1, b + 1, 1), x3 = P(a, b + 1, 0), y3 = P(a, b + 1, 1);
  const double sx = x0 - x1 + x2 - x3, sy = y0 - y1 + y2 - y3, dx1 = x1 - x2, dx2 = x3 - x2, dy1 = y1 - y2, dy2 = y3 - y2;
  const double den = dx1 * dy2 - dx2 * dy1, gg = (sx * dy2 - dx2 * sy) / den, hh = (dx1 * sy - sx * dy1) / den;
  const double A0 = x1 - x0 + gg * x1, A1 = x3 - x0 + hh * x3, A3 = y1 - y0 + gg * y1, A4 = y3 - y0 + hh * y3;
  const float* I = blurred + int64_t(G.frame) * h * w;
  auto at = [&](double du, double dv) {
    const double s = 0.5 + du, t = 0.5 + dv, q = gg * s + hh * t + 1.0;
    return bilin(I, w, h, (A0 * s + A1 * t + x0) / q, (A3 * s + A4 * t + y0) / q);
  };
  constexpr double kPi = 3.14159265358979323846;
  double dsum = at(0.0, 0.0);
  for (int q = 0; q < 4; ++q) dsum += at(0.07 * cos(q * kPi / 2), 0.07 * sin(q * kPi / 2));
  double rsum = 0.0;
  for (int q = 0; q < 8; ++q) rsum += at(0.32 * cos(q * kPi / 4), 0.32 * sin(q * kPi / 4));
  disc[cell] = dsum / 5.0;
  ring[cell] = rsum / 8.0;
}

// ---- host: grid assembly (tests/board_restatement.py assemble / marker_ids / ids_from_marker) --------------------------
struct V2 { double x, y; };
inline V2 operator-(V2 a, V2 b) { return {a.x - b.x, a.y - b.y}; }
inline V2 operator+(V2 a, V2 b) { return {a.x + b.x, a.y + b.y}; }
inline double nrm(V2 a) { return std::hypot(a.x, a.y); }

const int kDX[4] = {1, 1, 0, -1}, kDY[4] = {0, 1, 1, 1};

int pol_sign(int dir, V2 u, V2 v) {
  const double dx = kDX[dir], dy = kDY[dir], det = u.x * v.y - u.y * v.x;
  if (std::fabs(det) < 1e-12) return 0;
  const double al = (dx * v.y - dy * v.x) / det, be = (u.x * dy - u.y * dx) / det;
  return al * be > 0 ? 1 : -1;
}

// DLT homography (h33 = 1) from grid indices to pixels on centred, scaled points; solved by Gaussian elimination
bool homography(const std::vector<V2>& src, const std::vector<V2>& dst, double Hm[9]) {
  const size_t n = src.size();
  V2 ms{0, 0}, md{0, 0};
  for (size_t i = 0; i < n; ++i) { ms.x += src[i].x; ms.y += src[i].y; md.x += dst[i].x; md.y += dst[i].y; }
  ms.x /= n; ms.y /= n; md.x /= n; md.y /= n;
  double ss = 1e-12, sd = 1e-12;
  for (size_t i = 0; i < n; ++i) {
    ss = std::max({ss, std::fabs(src[i].x - ms.x), std::fabs(src[i].y - ms.y)});
    sd = std::max({sd, std::fabs(dst[i].x - md.x), std::fabs(dst[i].y - md.y)});
  }
  double M[8][9] = {};
  for (size_t i = 0; i < n; ++i) {
    const double x = (src[i].x - ms.x) / ss, y = (src[i].y - ms.y) / ss, u = (dst[i].x - md.x) / sd, v = (dst[i].y - md.y) / sd;
    const double r1[9] = {x, y, 1, 0, 0, 0, -u * x, -u * y, u}, r2[9] = {0, 0, 0, x, y, 1, -v * x, -v * y, v};
    for (int a = 0; a < 8; ++a) for (int b = 0; b < 9; ++b) M[a][b] += r1[a] * r1[b] + r2[a] * r2[b];
  }
  for (int a = 0; a < 8; ++a) M[a][a] += 1e-12;
  for (int c = 0; c < 8; ++c) {
    int p = c;
    for (int r = c + 1; r < 8; ++r) if (std::fabs(M[r][c]) > std::fabs(M[p][c])) p = r;
    if (std::fabs(M[p][c]) < 1e-300) return false;
    for (int b = 0; b < 9; ++b) std::swap(M[c][b], M[p][b]);
    for (int r = 0; r < 8; ++r) {
      if (r == c) continue;
      const double q = M[r][c] / M[c][c];
      for (int b = c; b < 9; ++b) M[r][b] -= q * M[c][b];
    }
  }
  double h[9];
  for (int a = 0; a < 8; ++a) h[a] = M[a][8] / M[a][a];
  h[8] = 1.0;
  // T2 * Hn * T1
  const double T1[9] = {1 / ss, 0, -ms.x / ss, 0, 1 / ss, -ms.y / ss, 0, 0, 1}, T2[9] = {sd, 0, md.x, 0, sd, md.y, 0, 0, 1};
  double t[9] = {};
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) for (int k = 0; k < 3; ++k) t[3 * i + j] += h[3 * i + k] * T1[3 * k + j];
  for (int i = 0; i < 9; ++i) Hm[i] = 0;
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) for (int k = 0; k < 3; ++k) Hm[3 * i + j] += T2[3 * i + k] * t[3 * k + j];
  return true;
}

V2 apply(const double Hm[9], double a, double b) {
  const double z = Hm[6] * a + Hm[7] * b + Hm[8];
  return {(Hm[0] * a + Hm[1] * b + Hm[2]) / z, (Hm[3] * a + Hm[4] * b + Hm[5]) / z};
}

struct Grid { int A = 0, B = 0; std::vector<int> idx; };   // idx[a*B + b]: index into the frame's candidate list

bool polarity_alternates(const std::vector<V2>& P, const std::vector<int>& pol, const Grid& G) {
  int ref = 0;
  for (int a = 0; a < G.A; ++a)
    for (int b = 0; b < G.B; ++b) {
      auto at = [&](int i, int j) { return P[size_t(G.idx[size_t(i * G.B + j)])]; };
      const V2 u = at(std::min(a + 1, G.A - 1), b) - at(std::max(a - 1, 0), b);
      const V2 v = at(a, std::min(b + 1, G.B - 1)) - at(a, std::max(b - 1, 0));
      const int s = pol_sign(pol[size_t(G.idx[size_t(a * G.B + b)])], u, v) * ((a + b) % 2 == 0 ? 1 : -1);
      if (s == 0 || (ref != 0 && s != ref)) return false;
      ref = s;
    }
  return true;
}

// cands sorted in raster order (the restatement's order); returns false when no W x H grid is found
bool assemble(const std::vector<V2>& pts, const std::vector<int>& pol, const std::vector<float>& resp, int W, int H, Grid* out) {
  const int n = int(pts.size());
  std::vector<int> order(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) order[size_t(i)] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return resp[size_t(a)] > resp[size_t(b)]; });
  std::vector<int> kept;
  for (int i : order) {
    bool ok = true;
    for (int j : kept) if (nrm(pts[size_t(i)] - pts[size_t(j)]) < 1.0) { ok = false; break; }
    if (ok) kept.push_back(i);
  }
  const int m = int(kept.size());
  if (m < W * H) return false;
  std::vector<V2> P(static_cast<size_t>(m)); std::vector<int> pl(static_cast<size_t>(m));
  for (int i = 0; i < m; ++i) { P[size_t(i)] = pts[size_t(kept[size_t(i)])]; pl[size_t(i)] = pol[size_t(kept[size_t(i)])]; }
  const int lim = std::max(W, H);
  for (int s0 = 0; s0 < std::min(8, m); ++s0) {
    std::vector<int> nn;
    for (int j = 0; j < m; ++j) if (j != s0) nn.push_back(j);
    std::stable_sort(nn.begin(), nn.end(), [&](int a, int b) { return nrm(P[size_t(a)] - P[size_t(s0)]) < nrm(P[size_t(b)] - P[size_t(s0)]); });
    const int c1 = nn[0];
    const V2 u = P[size_t(c1)] - P[size_t(s0)];
    const double du = nrm(u);
    int c2 = -1;
    for (size_t q = 1; q < nn.size(); ++q) {
      const V2 v = P[size_t(nn[q])] - P[size_t(s0)];
      const double dv = nrm(v);
      if (dv > 2.0 * du) break;
      if (std::fabs(u.x * v.x + u.y * v.y) < 0.6 * du * dv) { c2 = nn[q]; break; }
    }
    if (c2 < 0) continue;
    const V2 v = P[size_t(c2)] - P[size_t(s0)];
    const V2 pred = P[size_t(s0)] + u + v;
    int c3 = 0; double d3 = 1e300;
    for (int j = 0; j < m; ++j) { const double d = nrm(P[size_t(j)] - pred); if (d < d3) { d3 = d; c3 = j; } }
    if (d3 > 0.3 * std::min(du, nrm(v)) || c3 == s0 || c3 == c1 || c3 == c2) continue;
    const int g0 = pol_sign(pl[size_t(s0)], u, v), g1 = pol_sign(pl[size_t(c1)], u, v), g2 = pol_sign(pl[size_t(c2)], u, v), g3 = pol_sign(pl[size_t(c3)], u, v);
    if (!(g0 == g3 && g0 != 0 && g1 == g2 && g1 == -g0)) continue;
    std::map<std::pair<int, int>, int> grid{{{0, 0}, s0}, {{1, 0}, c1}, {{0, 1}, c2}, {{1, 1}, c3}};
    std::set<int> used{s0, c1, c2, c3};
    bool ok = true;
    while (true) {
      int amin = 1 << 30, amax = -(1 << 30), bmin = 1 << 30, bmax = -(1 << 30);
      for (const auto& kv : grid) { amin = std::min(amin, kv.first.first); amax = std::max(amax, kv.first.first); bmin = std::min(bmin, kv.first.second); bmax = std::max(bmax, kv.first.second); }
      if (amax - amin + 1 > lim || bmax - bmin + 1 > lim) { ok = false; break; }
      std::set<std::pair<int, int>> front;
      const int da[4] = {1, -1, 0, 0}, db[4] = {0, 0, 1, -1};
      for (const auto& kv : grid) for (int q = 0; q < 4; ++q) {
        const std::pair<int, int> p{kv.first.first + da[q], kv.first.second + db[q]};
        if (!grid.count(p)) front.insert(p);
      }
      bool changed = false;
      for (const auto& p : front) {
        std::vector<V2> src, dst; std::set<int> as, bs;
        for (const auto& kv : grid)
          if (std::abs(kv.first.first - p.first) <= 2 && std::abs(kv.first.second - p.second) <= 2) {
            src.push_back({double(kv.first.first), double(kv.first.second)}); dst.push_back(P[size_t(kv.second)]);
            as.insert(kv.first.first); bs.insert(kv.first.second);
          }
        if (src.size() < 4 || as.size() < 2 || bs.size() < 2) continue;
        double Hm[9];
        if (!homography(src, dst, Hm)) continue;
        const V2 pr = apply(Hm, p.first, p.second);
        const double sl = std::min(nrm(apply(Hm, p.first + 1, p.second) - pr), nrm(apply(Hm, p.first, p.second + 1) - pr));
        int j = 0; double dj = 1e300;
        for (int q = 0; q < m; ++q) { const double d = nrm(P[size_t(q)] - pr); if (d < dj) { dj = d; j = q; } }
        if (dj < 0.3 * sl && !used.count(j)) { grid[p] = j; used.insert(j); changed = true; }
      }
      if (!changed) break;
    }
    if (!ok) continue;
    int amin = 1 << 30, amax = -(1 << 30), bmin = 1 << 30, bmax = -(1 << 30);
    for (const auto& kv : grid) { amin = std::min(amin, kv.first.first); amax = std::max(amax, kv.first.first); bmin = std::min(bmin, kv.first.second); bmax = std::max(bmax, kv.first.second); }
    const int A = amax - amin + 1, B = bmax - bmin + 1;
    if (!((A == W && B == H) || (A == H && B == W)) || int(grid.size()) != A * B) continue;
    Grid G; G.A = A; G.B = B; G.idx.assign(size_t(A * B), 0);
    for (const auto& kv : grid) G.idx[size_t((kv.first.first - amin) * B + (kv.first.second - bmin))] = kv.second;
    if (!polarity_alternates(P, pl, G)) continue;
    for (int& i : G.idx) i = kept[size_t(i)];
    *out = G;
    return true;
  }
  return false;
}

// marker_ids + ids_from_marker: ids[a*B + b], or false
bool marker_ids(const Grid& G, const std::vector<V2>& pts, const double* disc, const double* ring, int W, int H, std::vector<int>* ids) {
  const int nc = (G.A - 1) * (G.B - 1);
  double rmax = -1e300, rmin = 1e300;
  for (int k = 0; k < nc; ++k) { rmax = std::max(rmax, ring[k]); rmin = std::min(rmin, ring[k]); }
  const double mid = 0.5 * (rmax + rmin);
  double sw = 0, sb = 0; int nw = 0, nb = 0;
  for (int k = 0; k < nc; ++k) { if (ring[k] > mid) { sw += ring[k]; ++nw; } else { sb += ring[k]; ++nb; } }
  if (nw == 0 || nb == 0) return false;
  const double contrast = sw / nw - sb / nb;
  if (contrast <= 0) return false;
  std::vector<std::array<int, 2>> bl, wh;
  for (int k = 0; k < nc; ++k) {
    const bool white = ring[k] > mid;
    const double score = (ring[k] - disc[k]) / contrast;
    const std::array<int, 2> c{k / (G.B - 1), k % (G.B - 1)};
    if (white && score > 0.5) bl.push_back(c);
    if (!white && score < -0.5) wh.push_back(c);
  }
  if (bl.size() != 1 || wh.size() != 2) return false;
  const std::array<int, 2> bc = bl[0];
  std::array<int, 2> d[2];
  for (int q = 0; q < 2; ++q) {
    d[q] = {wh[size_t(q)][0] - bc[0], wh[size_t(q)][1] - bc[1]};
    if (std::abs(d[q][0]) + std::abs(d[q][1]) != 1) return false;
  }
  if (d[0][0] * d[1][0] + d[0][1] * d[1][1] != 0) return false;
  auto P = [&](int a, int b) { return pts[size_t(G.idx[size_t(a * G.B + b)])]; };
  auto cen = [&](std::array<int, 2> c) {
    const V2 s = P(c[0], c[1]) + P(c[0] + 1, c[1]) + P(c[0], c[1] + 1) + P(c[0] + 1, c[1] + 1);
    return V2{s.x / 4, s.y / 4};
  };
  const V2 pb = cen(bc);
  std::array<int, 2> up{0, 0}, right{0, 0};
  bool found = false;
  for (int q = 0; q < 2 && !found; ++q) {
    up = d[q]; right = d[1 - q];
    const V2 ri = cen({bc[0] + right[0], bc[1] + right[1]}) - pb, dn = pb - cen({bc[0] + up[0], bc[1] + up[1]});
    found = ri.x * dn.y - ri.y * dn.x > 0;
  }
  if (!found) return false;
  const int row[2] = {-up[0], -up[1]}, col[2] = {right[0], right[1]};
  const int r0 = (H - 1) / 2, c0 = W / 2 - 1;
  // the origin: the corner of the black-dot square with the smallest (row, column)
  const std::array<int, 2> cells[4] = {{bc[0], bc[1]}, {bc[0] + 1, bc[1]}, {bc[0], bc[1] + 1}, {bc[0] + 1, bc[1] + 1}};
  std::array<int, 2> o = cells[0];
  for (const auto& c : cells) {
    const int kr = row[0] * c[0] + row[1] * c[1], kc = col[0] * c[0] + col[1] * c[1];
    const int orr = row[0] * o[0] + row[1] * o[1], oc = col[0] * o[0] + col[1] * o[1];
    if (kr < orr || (kr == orr && kc < oc)) o = c;
  }
  ids->assign(size_t(G.A * G.B), 0);
  for (int a = 0; a < G.A; ++a)
    for (int b = 0; b < G.B; ++b) {
      const int qa = a - o[0], qb = b - o[1];
      const int i = r0 + row[0] * qa + row[1] * qb, j = c0 + col[0] * qa + col[1] * qb;
      if (i < 0 || i >= H || j < 0 || j >= W) return false;
      (*ids)[size_t(a * G.B + b)] = i * W + j;
    }
  return true;
}

void resize_axis(int n_src, double factor, int* n_dst, std::vector<int>* idx, std::vector<int>* w1) {
  const double f = 1.0 / factor, scale = 1.0 / f;
  *n_dst = int(std::nearbyint(n_src * f));
  idx->assign(size_t(std::max(*n_dst, 0)), 0); w1->assign(size_t(std::max(*n_dst, 0)), 0);
  for (int x = 0; x < *n_dst; ++x) {
    const double sx = (x + 0.5) * scale - 0.5;
    int s0 = int(std::floor(sx));
    double fx = sx - s0;
    if (s0 < 0) { s0 = 0; fx = 0.0; }
    if (s0 >= n_src - 1) { s0 = n_src - 1; fx = 0.0; }
    (*idx)[size_t(x)] = s0;
    (*w1)[size_t(x)] = int(std::floor(fx * 2048.0 + 0.5));
  }
}

struct Slot {
  oicc::PinnedBuf<uint8_t> pinned;
  oicc::DevBuf<uint8_t> d_src, d_gray, d_pol;
  oicc::DevBuf<float> d_resp, d_blur;
  oicc::DevBuf<unsigned int> d_max;
  oicc::DevBuf<int> d_count;
  oicc::DevBuf<Cand> d_cand;
  oicc::DevBuf<double> d_ref;
  oicc::DevBuf<GridRef> d_gr; oicc::DevBuf<double> d_gc, d_disc, d_ring;    // kernel 6: grown to the batch's grids, kept for the slot's next batch
  oicc::Event up, ev[6], done;
};

}  // namespace

extern "C" int oicc_board_output_size(int32_t width, int32_t height, double downsample_factor, int32_t* out_width, int32_t* out_height) {
  if (width <= 0 || height <= 0 || !(downsample_factor > 0) || !out_width || !out_height) return OICC_ERR_INVALID_ARG;
  std::vector<int> a, b;
  int wd = 0, hd = 0;
  resize_axis(width, downsample_factor, &wd, &a, &b);
  resize_axis(height, downsample_factor, &hd, &a, &b);
  *out_width = wd; *out_height = hd;
  return OICC_OK;
}

extern "C" int oicc_board_radon_detect(int32_t device_ordinal, int32_t num_frames, int32_t width, int32_t height, int32_t channels,
                                       const uint8_t* frames, double downsample_factor, int32_t W, int32_t H,
                                       const oicc_board_options* opt, double* corners, int32_t* found, int32_t* candidates_per_frame,
                                       oicc_board_report* report, const oicc_board_stages* stages) {
  if (num_frames < 0 || width <= 0 || height <= 0 || (channels != 1 && channels != 3) || (!frames && num_frames > 0) ||
      !(downsample_factor > 0) || W < 2 || H < 2 || !opt || !corners || !found) return OICC_ERR_INVALID_ARG;
  const int r = opt->radius, cap = opt->max_candidates, batch = opt->batch > 0 ? opt->batch : 64;
  if (r < 1 || r > kMaxRadius || cap < W * H || cap > (1 << 16) || opt->subpix_iterations < 0 || !(opt->threshold_rel >= 0)) return OICC_ERR_INVALID_ARG;
  int wd = 0, hd = 0;
  std::vector<int> xi, xw, yi, yw;
  resize_axis(width, downsample_factor, &wd, &xi, &xw);
  resize_axis(height, downsample_factor, &hd, &yi, &yw);
  if (wd < 2 * r + 3 || hd < 2 * r + 3) return OICC_ERR_INVALID_ARG;
  if (int rc = oicc::select_device(device_ordinal)) return rc;
  oicc_board_report rep;
  std::memset(&rep, 0, sizeof(rep));
  const auto t_start = std::chrono::steady_clock::now();
  const int64_t in_frame = int64_t(width) * height * channels, out_frame = int64_t(wd) * hd;
  const int64_t nbatch = std::min<int64_t>(batch, std::max(num_frames, 1));
  const int nslots = num_frames > nbatch ? 2 : 1;     // a second staging slot only when a second batch exists
  const int WH = W * H;
  const float inv = float(1.0 / (16.0 * 255.0 * (2 * r + 1)));
  const int win = r + 2;
  const oicc_board_stages* ext = stages && stages->extended ? stages : nullptr;     // the fields behind `extended` exist only then
  std::vector<int> tab;
  for (int i = 0; i < num_frames * WH * 2; ++i) corners[i] = std::nan("");
  for (int i = 0; i < num_frames; ++i) { found[i] = 0; if (candidates_per_frame) candidates_per_frame[i] = 0; }
  tab.insert(tab.end(), xi.begin(), xi.end()); tab.insert(tab.end(), xw.begin(), xw.end());
  tab.insert(tab.end(), yi.begin(), yi.end()); tab.insert(tab.end(), yw.begin(), yw.end());
  // the device work in a scope of its own: its streams and buffers are gone before ms_total is taken and the report written
  const int rc = [&]() -> int {
    oicc::DevBuf<int> d_tab_buf;
    Slot slot[2];
    std::vector<GridRef> gr; std::vector<double> gc, disc, ring;      // kernel 6's arguments and results: asynchronous copies on ks read and write them
    oicc::Stream cs, ks;      // behind every buffer and event their work uses (hip_resources.h)
    OICC_HIP_TRY(cs.create());
    OICC_HIP_TRY(ks.create());
    OICC_HIP_TRY(d_tab_buf.resize(tab.size()));
    const int* d_tab = d_tab_buf.p;
    OICC_HIP_TRY(hipMemcpy(d_tab_buf.p, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice));
    for (int q = 0; q < nslots; ++q) {
      Slot& s = slot[q];
      OICC_HIP_TRY(s.pinned.alloc(size_t(nbatch * in_frame)));
      OICC_HIP_TRY(s.d_src.resize(size_t(nbatch * in_frame)));
      OICC_HIP_TRY(s.d_gray.resize(size_t(nbatch * out_frame)));
      OICC_HIP_TRY(s.d_resp.resize(size_t(nbatch * out_frame)));
      OICC_HIP_TRY(s.d_pol.resize(size_t(nbatch * out_frame)));
      OICC_HIP_TRY(s.d_blur.resize(size_t(nbatch * out_frame)));
      OICC_HIP_TRY(s.d_max.resize(size_t(nbatch)));
      OICC_HIP_TRY(s.d_count.resize(size_t(nbatch)));
      OICC_HIP_TRY(s.d_cand.resize(size_t(nbatch * cap)));
      OICC_HIP_TRY(s.d_ref.resize(2 * size_t(nbatch * cap)));
      OICC_HIP_TRY(s.up.create()); OICC_HIP_TRY(s.done.create());
      for (auto& e : s.ev) OICC_HIP_TRY(e.create());
    }
    // enqueue: host copy into the slot's pinned buffer, upload on the copy stream, kernels 1-4 on the compute stream
    auto enqueue = [&](int q, int first, int num) -> int {
      Slot& s = slot[q];
      OICC_HIP_TRY(hipEventSynchronize(s.done));
      std::memcpy(s.pinned.p, frames + int64_t(first) * in_frame, size_t(num * in_frame));
      OICC_HIP_TRY(hipMemcpyAsync(s.d_src.p, s.pinned.p, size_t(num * in_frame), hipMemcpyHostToDevice, cs));
      OICC_HIP_TRY(hipEventRecord(s.up, cs));
      OICC_HIP_TRY(hipStreamWaitEvent(ks, s.up, 0));
      OICC_HIP_TRY(hipMemsetAsync(s.d_max.p, 0, sizeof(unsigned int) * size_t(num), ks));
      OICC_HIP_TRY(hipMemsetAsync(s.d_count.p, 0, sizeof(int) * size_t(num), ks));
      OICC_HIP_TRY(hipEventRecord(s.ev[0], ks));
      board_resize_gray_kernel<<<dim3((wd + kThreads - 1) / kThreads, hd, num), kThreads, 0, ks>>>(
          s.d_src.p, width, height, channels, wd, hd, d_tab, d_tab + wd, d_tab + 2 * wd, d_tab + 2 * wd + hd, s.d_gray.p);
      OICC_HIP_TRY(hipEventRecord(s.ev[1], ks));
      board_response_kernel<<<dim3((wd + kTileX - 1) / kTileX, (hd + kTileY - 1) / kTileY, num), kThreads, 0, ks>>>(
          s.d_gray.p, wd, hd, r, inv, s.d_resp.p, s.d_pol.p, s.d_blur.p, s.d_max.p);
      OICC_HIP_TRY(hipEventRecord(s.ev[2], ks));
      board_candidates_kernel<<<dim3((wd + kThreads - 1) / kThreads, hd, num), kThreads, 0, ks>>>(
          s.d_resp.p, s.d_pol.p, wd, hd, r, opt->threshold_rel, s.d_max.p, cap, s.d_count.p, s.d_cand.p);
      OICC_HIP_TRY(hipEventRecord(s.ev[3], ks));
      const int64_t waves = int64_t(num) * cap;
      board_subpix_kernel<<<dim3(unsigned((waves + 3) / 4)), kThreads, 0, ks>>>(s.d_blur.p, wd, hd, num, cap, s.d_count.p, s.d_cand.p, win,
                                                                               opt->subpix_iterations, opt->subpix_eps, s.d_ref.p);
      OICC_HIP_TRY(hipGetLastError());
      OICC_HIP_TRY(hipEventRecord(s.ev[4], ks));
      OICC_HIP_TRY(hipEventRecord(s.done, ks));
      return OICC_OK;
    };
    // complete: the batch's candidates to the host, grids assembled there, kernel 6 over them, the corners written
    auto complete = [&](int q, int first, int num) -> int {
      Slot& s = slot[q];
      OICC_HIP_TRY(hipEventSynchronize(s.done));
      float ms = 0;
      double* acc[4] = {&rep.ms_resize, &rep.ms_response, &rep.ms_candidates, &rep.ms_subpix};
      for (int j = 0; j < 4; ++j) { OICC_HIP_TRY(hipEventElapsedTime(&ms, s.ev[j], s.ev[j + 1])); *acc[j] += ms; }
      std::vector<int> cnt(static_cast<size_t>(num));
      std::vector<Cand> cand(size_t(num) * cap);
      std::vector<double> ref(size_t(num) * cap * 2);
      OICC_HIP_TRY(hipMemcpy(cnt.data(), s.d_count.p, sizeof(int) * cnt.size(), hipMemcpyDeviceToHost));
      OICC_HIP_TRY(hipMemcpy(cand.data(), s.d_cand.p, sizeof(Cand) * cand.size(), hipMemcpyDeviceToHost));
      OICC_HIP_TRY(hipMemcpy(ref.data(), s.d_ref.p, sizeof(double) * ref.size(), hipMemcpyDeviceToHost));
      if (stages) {
        for (int f = 0; f < num; ++f) {
          const int64_t F = first + f;
          if (stages->gray) OICC_HIP_TRY(hipMemcpy(stages->gray + F * out_frame, s.d_gray.p + f * out_frame, size_t(out_frame), hipMemcpyDeviceToHost));
          if (stages->response) OICC_HIP_TRY(hipMemcpy(stages->response + F * out_frame, s.d_resp.p + f * out_frame, sizeof(float) * size_t(out_frame), hipMemcpyDeviceToHost));
          if (ext && ext->polarity) OICC_HIP_TRY(hipMemcpy(ext->polarity + F * out_frame, s.d_pol.p + f * out_frame, size_t(out_frame), hipMemcpyDeviceToHost));
          if (ext && ext->blurred) OICC_HIP_TRY(hipMemcpy(ext->blurred + F * out_frame, s.d_blur.p + f * out_frame, sizeof(float) * size_t(out_frame), hipMemcpyDeviceToHost));
          if (ext && ext->grid_shape) { ext->grid_shape[2 * F] = 0; ext->grid_shape[2 * F + 1] = 0; }
        }
      }
      const auto th0 = std::chrono::steady_clock::now();
      // per frame: candidates in raster order, then the grid
      std::vector<std::vector<V2>> fpts(static_cast<size_t>(num));
      std::vector<Grid> grids(static_cast<size_t>(num));
      std::vector<char> has(static_cast<size_t>(num), 0);
      for (int f = 0; f < num; ++f) {
        const int n = cnt[size_t(f)], F = first + f;
        if (candidates_per_frame) candidates_per_frame[F] = n;
        rep.num_candidates += n;
        if (n > cap) { ++rep.frames_overflow; continue; }
        std::vector<int> ord(static_cast<size_t>(n));
        for (int i = 0; i < n; ++i) ord[size_t(i)] = i;
        const Cand* c = cand.data() + size_t(f) * cap;
        std::sort(ord.begin(), ord.end(), [&](int a, int b) { return c[a].y != c[b].y ? c[a].y < c[b].y : c[a].x < c[b].x; });
        std::vector<V2> pts; std::vector<int> pol; std::vector<float> rs;
        for (int i : ord) {
          pts.push_back({ref[2 * (size_t(f) * cap + size_t(i))], ref[2 * (size_t(f) * cap + size_t(i)) + 1]});
          pol.push_back(c[i].pol); rs.push_back(c[i].resp);
          if (stages && stages->candidates && stages->refined && stages->capacity > 0) {
            const int q = int(pts.size()) - 1;
            if (q < stages->capacity) {
              stages->candidates[2 * (int64_t(F) * stages->capacity + q)] = c[i].x; stages->candidates[2 * (int64_t(F) * stages->capacity + q) + 1] = c[i].y;
              stages->refined[2 * (int64_t(F) * stages->capacity + q)] = pts.back().x; stages->refined[2 * (int64_t(F) * stages->capacity + q) + 1] = pts.back().y;
            }
          }
        }
        fpts[size_t(f)] = pts;
        if (n >= WH && assemble(pts, pol, rs, W, H, &grids[size_t(f)])) has[size_t(f)] = 1;
        if (ext && has[size_t(f)]) {
          const Grid& G = grids[size_t(f)];
          if (ext->grid_shape) { ext->grid_shape[2 * int64_t(F)] = G.A; ext->grid_shape[2 * int64_t(F) + 1] = G.B; }
          if (ext->grid) std::copy(G.idx.begin(), G.idx.end(), ext->grid + int64_t(F) * WH);
        }
      }
      rep.ms_assembly_host += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th0).count();
      // kernel 6 over every assembled grid of the batch
      gr.clear(); gc.clear();
      int ncell = 0;
      for (int f = 0; f < num; ++f) {
        if (!has[size_t(f)]) continue;
        const Grid& G = grids[size_t(f)];
        gr.push_back(GridRef{f, G.A, G.B, int(gc.size() / 2), ncell});
        for (int i : G.idx) { gc.push_back(fpts[size_t(f)][size_t(i)].x); gc.push_back(fpts[size_t(f)][size_t(i)].y); }
        ncell += (G.A - 1) * (G.B - 1);
      }
      if (!gr.empty()) {
        disc.assign(size_t(ncell), 0.0); ring.assign(size_t(ncell), 0.0);
        OICC_HIP_TRY(s.d_gr.resize(gr.size())); OICC_HIP_TRY(s.d_gc.resize(gc.size()));
        OICC_HIP_TRY(s.d_disc.resize(size_t(ncell))); OICC_HIP_TRY(s.d_ring.resize(size_t(ncell)));
        OICC_HIP_TRY(hipMemcpyAsync(s.d_gr.p, gr.data(), sizeof(GridRef) * gr.size(), hipMemcpyHostToDevice, ks));
        OICC_HIP_TRY(hipMemcpyAsync(s.d_gc.p, gc.data(), sizeof(double) * gc.size(), hipMemcpyHostToDevice, ks));
        OICC_HIP_TRY(hipEventRecord(s.ev[4], ks));
        board_marker_kernel<<<dim3((ncell + kThreads - 1) / kThreads), kThreads, 0, ks>>>(s.d_blur.p, wd, hd, int(gr.size()), s.d_gr.p, s.d_gc.p, ncell, s.d_disc.p, s.d_ring.p);
        OICC_HIP_TRY(hipGetLastError());
        OICC_HIP_TRY(hipEventRecord(s.ev[5], ks));
        OICC_HIP_TRY(hipMemcpyAsync(disc.data(), s.d_disc.p, sizeof(double) * size_t(ncell), hipMemcpyDeviceToHost, ks));
        OICC_HIP_TRY(hipMemcpyAsync(ring.data(), s.d_ring.p, sizeof(double) * size_t(ncell), hipMemcpyDeviceToHost, ks));
        OICC_HIP_TRY(hipStreamSynchronize(ks));
        OICC_HIP_TRY(hipEventElapsedTime(&ms, s.ev[4], s.ev[5]));
        rep.ms_marker += ms;
        const auto th1 = std::chrono::steady_clock::now();
        for (const GridRef& g : gr) {
          const Grid& G = grids[size_t(g.frame)];
          const int nc = (G.A - 1) * (G.B - 1);
          if (ext && ext->disc) std::copy(disc.begin() + g.cell0, disc.begin() + g.cell0 + nc, ext->disc + int64_t(first + g.frame) * nc);
          if (ext && ext->ring) std::copy(ring.begin() + g.cell0, ring.begin() + g.cell0 + nc, ext->ring + int64_t(first + g.frame) * nc);
          std::vector<int> ids;
          if (!marker_ids(G, fpts[size_t(g.frame)], disc.data() + g.cell0, ring.data() + g.cell0, W, H, &ids)) continue;
          const int F = first + g.frame;
          for (size_t q = 0; q < ids.size(); ++q) {
            const V2 p = fpts[size_t(g.frame)][size_t(G.idx[q])];
            corners[2 * (int64_t(F) * WH + ids[q])] = p.x; corners[2 * (int64_t(F) * WH + ids[q]) + 1] = p.y;
          }
          found[F] = 1; ++rep.frames_found;
        }
        rep.ms_assembly_host += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th1).count();
      }
      return OICC_OK;
    };
    for (int q = 0; q < nslots; ++q) OICC_HIP_TRY(hipEventRecord(slot[q].done, ks));
    return oicc::run_frame_batches(num_frames, int(nbatch), enqueue, complete);
  }();
  rep.output_width = wd; rep.output_height = hd;
  rep.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
  if (report) *report = rep;
  return rc;
}
