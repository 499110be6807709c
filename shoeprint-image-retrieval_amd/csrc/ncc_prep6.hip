// Gallery preparation of the six-wave FFT layout for the corner-window case (template at least as large as the
// search map: th >= ih and tw >= iw, which is every plan whose queries and gallery share a size).
//
// Same prepared item as prep_fft_kernel writes (spectra, 1/sigma slice in Cfg::inv6_index order, dead flags), with
//   * one workgroup per (item, group of channels): the raw map of channel c+1 is requested into registers before the
//     statistics of channel c start, so only the first channel of a workgroup waits for HBM;
//   * mean, centred map and energy straight from those registers (element-to-lane mapping and reduction order of
//     load_centred / template_scale: the centred map, the scale and the dead flag are bit-identical);
//   * corner sums instead of two summed-area tables.  A 'same'-mode window of a template that covers the map is, along
//     each axis, a prefix [0, b) or a suffix [a, n) = total - prefix: one pass along the rows turns x and x^2 into
//     horizontal window sums, one pass down the columns turns those into the window sums, both on float64 prefixes
//     held in registers (a line is cut into four stretches on four lanes of one wave; the totals of the stretches
//     travel by lane exchange), and the 1/sigma slice is evaluated in slot order from two look-ups per sum and leaves
//     as 16-byte stores;
//   * the forward transforms of prep_fft_kernel, unchanged (bit-identical spectra).
#include "fft_core.h"
#include "ncc_fft_cfg.h"
#include "ncc_prep_common.h"

namespace spr {
namespace {

using C6 = Cfg<12, 16, 12, 8, 384, 5, 2, 1>;
constexpr int kPT = 512;         // work-items per workgroup (8 waves, one workgroup per CU)
constexpr int kLoads = 16;       // raw values per work-item (load_centred's batch): maps of up to 16 * 512 pixels
constexpr int kSeg = 4;          // stretches per row / column
constexpr int kRowSeg = 16;      // longest row stretch (w <= 64)
constexpr int kChansPerWg = 8;   // channels one workgroup walks: 1500 x 256 channels are 48 000 workgroups on 256 CUs

// -DSPR_PREP6_STAMPS (this file only): the diagnostic build for tools/ubench/stamps_prep.py - one workgroup records the
// shader clock at the phase boundaries of its second channel (the pipeline's steady state)
#ifdef SPR_PREP6_STAMPS
__device__ unsigned long long g_prep6_stamps[16];
#define SPR_PSTAMP6(i) do { if (blockIdx.x == 12 && blockIdx.y == 700 && c == c_first + 1 && threadIdx.x == 0) g_prep6_stamps[i] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define SPR_PSTAMP6(i)
#endif

struct Prep6Lds {
  size_t x0_off, f_off, xbuf_off, tw_off, total;
  int f_stride;
};
Prep6Lds prep6_lds(const NccGeom& g) {
  const int h = g.ih, w = g.iw;
  Prep6Lds l;
  l.f_stride = C6::NW / 2 + 1;
  const size_t f_bytes = sizeof(cf) * static_cast<size_t>(2 * ((h + 1) / 2)) * l.f_stride;
  l.x0_off = 64;
  l.f_off = align_up(l.x0_off + sizeof(float) * h * w, 16);
  l.xbuf_off = align_up(l.f_off + f_bytes, 16);
  const size_t fft_total = l.xbuf_off + sizeof(cf) * C6::prep_xbuf_elems(kPT);
  // the statistics' two float64 planes share the transforms' space
  const size_t stat_total = l.f_off + 2 * sizeof(double) * static_cast<size_t>(h) * w;
  l.tw_off = align_up(fft_total > stat_total ? fft_total : stat_total, 16);
  l.total = l.tw_off + sizeof(cf) * (C6::NW + C6::NH);
  return l;
}

// Offset of stretch sg (the totals of the stretches before it) and the total of the line, from the four stretch totals
// that the lanes l ^ d, l ^ 2d, l ^ 3d hold: every lane of the line adds them in the same order.
__device__ __forceinline__ void stretch_offsets(double t, int sg, int d, double& off, double& tot) {
  const double a = shfl_xor(t, d), b = shfl_xor(t, 2 * d), c = shfl_xor(t, 3 * d);
  off = 0.0;
  tot = 0.0;
#pragma unroll
  for (int j = 0; j < kSeg; ++j) {
    const double v = j == sg ? t : (j == (sg ^ 1) ? a : (j == (sg ^ 2) ? b : c));
    off += j < sg ? v : 0.0;
    tot += v;
  }
}

__global__ void __launch_bounds__(kPT)
prep6_gallery_kernel(NccGeom g, const void* __restrict__ maps, unsigned char* __restrict__ prepared, size_t item_bytes,
                     const cf* __restrict__ tw_h, const cf* __restrict__ tw_w, unsigned x0_off, unsigned f_off,
                     unsigned xbuf_off, unsigned tw_off, int f_stride) {
  using C = C6;
  using GH = typename C::GH;
  using GW = typename C::GW;
  unsigned char* lds = dyn_lds();
  double* red = reinterpret_cast<double*>(lds);
  float* x0 = reinterpret_cast<float*>(lds + x0_off);
  cf* F = reinterpret_cast<cf*>(lds + f_off);
  cf* xbuf = reinterpret_cast<cf*>(lds + xbuf_off);
  const int tid = static_cast<int>(threadIdx.x);
  const size_t item = blockIdx.y;
  const int h = g.ih, w = g.iw, n = h * w;
  double* H1 = reinterpret_cast<double*>(lds + f_off);  // horizontal window sums of x0 and of fl32(x0^2), [y][x]
  double* H2 = H1 + n;
  const int c_first = static_cast<int>(blockIdx.x) * kChansPerWg;
  const int c_end = c_first + kChansPerWg < g.channels ? c_first + kChansPerWg : g.channels;

  unsigned char* item_base = prepared + item * item_bytes;
  const size_t spec_bytes = sizeof(cf) * static_cast<size_t>(g.channels) * C::kSpecPerChan;
  unsigned char* flags = item_base + spec_bytes + sizeof(float) * static_cast<size_t>(g.channels) * g.inv_per_chan;

  // pixel i = tid + k * kPT of this work-item (load_centred's mapping)
  const int dy = kPT / w, dx = kPT - dy * w;
  const int y_first = tid / w, x_first = tid - y_first * w;
  float v[kLoads];
  auto request = [&](int c) {
    const size_t chan_base = (item * g.channels + c) * static_cast<size_t>(g.g_h) * g.g_w;
    int yy = y_first, xx = x_first;
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
      v[k] = tid + k * kPT < n
                 ? load_feature(maps, chan_base + static_cast<size_t>(yy + g.crop) * g.g_w + (xx + g.crop), g.dtype)
                 : 0.0f;
      xx += dx; yy += dy;
      if (xx >= w) { xx -= w; ++yy; }
    }
  };
  request(c_first);

  // forward twiddle tables w^(-t*p), [p][t], in LDS: read at use, no registers held across the channel loop
  cf* twt_w = reinterpret_cast<cf*>(lds + tw_off);
  cf* twt_h = twt_w + C::NW;
  for (int k = tid; k < C::NW; k += kPT) twt_w[k] = tw_w[(k / C::TGW) * (k % C::TGW)];
  for (int k = tid; k < C::NH; k += kPT) twt_h[k] = tw_h[(k / C::TGH) * (k % C::TGH)];

  const int cy = g.th / 2, cx = g.tw / 2;
  const int above = g.th - cy, left = g.tw - cx;  // a window starting at 0 ends at y + above / x + left (clipped)
  const double inv_n = 1.0 / (static_cast<double>(g.th) * static_cast<double>(g.tw));

  for (int c = c_first; c < c_end; ++c) {
    SPR_PSTAMP6(0);
    // ---- mean, centred map, energy: from the registers ------------------------------------------------------------
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < kLoads; ++k)
      if (tid + k * kPT < n) s += static_cast<double>(v[k]);
    const double total = block_sum(s, red);
    const float mean = static_cast<float>(total / static_cast<double>(n));
    double e = 0.0;
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
      if (tid + k * kPT < n) {
        const float d = v[k] - mean;
        x0[tid + k * kPT] = d;
        const float sq = d * d;  // np.square keeps float32 (similarity.py:67)
        e += static_cast<double>(sq);
      }
    }
    SPR_PSTAMP6(1);
    const float energy = static_cast<float>(block_sum(e, red));  // (its barriers publish x0)
    const float rs = energy > 0.0f ? static_cast<float>(1.0 / sqrt(static_cast<double>(energy))) : 0.0f;
    if (tid == 0) flags[c] = rs == 0.0f ? 1 : 0;
    if (c + 1 < c_end) request(c + 1);  // in flight through the statistics and the transforms of this channel
    SPR_PSTAMP6(2);

    // ---- rows: work-item (y, stretch) -> horizontal window sums ---------------------------------------------------
    {
      const int tidv = opaque(tid);  // lane coordinates are re-derived per phase: hoisted out of the channel loop they cost registers
      const int u = tidv < h * kSeg ? tidv : h * kSeg - 1;  // surplus lanes shadow the last unit (they take part in the exchange)
      const bool live = tidv < h * kSeg;
      const int y = u / kSeg, sg = u - y * kSeg;
      const int wseg = (w + kSeg - 1) / kSeg;
      const int xa = sg * wseg < w ? sg * wseg : w;
      const int cnt = w - xa < wseg ? w - xa : wseg;  // 0: a stretch past the last column of a narrow map
      const float* src = x0 + y * w;
      float tv[kRowSeg];  // the stretch in registers: one LDS round trip, zeros past its end
#pragma unroll
      for (int k = 0; k < kRowSeg; ++k) {
        const float t = src[xa + k < w ? xa + k : w - 1];
        tv[k] = k < cnt ? t : 0.0f;
      }
      double r1 = 0.0, r2 = 0.0;  // totals of the stretch
#pragma unroll
      for (int k = 0; k < kRowSeg; ++k) {
        const float sq = tv[k] * tv[k];  // np.square keeps float32 (similarity.py:57)
        r1 += static_cast<double>(tv[k]);
        r2 += static_cast<double>(sq);
      }
      double q1, q2, t1, t2;  // running prefixes of the row, from the totals of the stretches before this one; row totals
      stretch_offsets(r1, sg, 1, q1, t1);
      stretch_offsets(r2, sg, 1, q2, t2);
      double* h1 = H1 + y * w;
      double* h2 = H2 + y * w;
      if (live) {
#pragma unroll
        for (int k = 0; k < kRowSeg; ++k) {
          const float sq = tv[k] * tv[k];
          q1 += static_cast<double>(tv[k]);
          q2 += static_cast<double>(sq);
          const int kk = xa + k + 1;  // prefix [0, kk) of the row
          if (k < cnt && kk < w) {
            const int xl = kk - left;  // the window of pixel xl is that prefix
            if (xl >= 0 && xl <= cx) { h1[xl] = q1; h2[xl] = q2; }
            const int xr = kk + cx;    // the window of pixel xr is the rest of the row
            if (xr < w) { h1[xr] = t1 - q1; h2[xr] = t2 - q2; }
          }
        }
        if (cnt > 0 && xa + cnt == w) {  // the whole row (q = its total now): every pixel whose window starts at 0 and
          int xl = w - left < 0 ? 0 : w - left;  // reaches the last column
          const int xe = cx < w - 1 ? cx : w - 1;
          for (; xl <= xe; ++xl) { h1[xl] = q1; h2[xl] = q2; }
        }
      }
    }
    __syncthreads();
    SPR_PSTAMP6(7);

    // ---- columns: lane (plane, column, stretch) - waves 0-3 take the plane of x0, waves 4-7 that of x0^2.  Each plane
    // becomes its vertical prefixes, P[y][x] = sum of rows <= y, in place; the four stretches of a column sit 16 lanes apart
    {
      const int tidv = opaque(tid);
      const int xcol = ((tidv >> 6) & 3) * 16 + (tidv & 15), csg = (tidv >> 4) & 3;
      const int hseg = (h + kSeg - 1) / kSeg;
      const int ya = csg * hseg < h ? csg * hseg : h;
      const int ycnt = xcol < w ? (h - ya < hseg ? h - ya : hseg) : 0;  // surplus lanes only take part in the exchange
      double* col = ((tidv >> 8) ? H2 : H1) + ya * w + (xcol < w ? xcol : w - 1);
      constexpr int B = 8;  // one LDS round trip per batch
      double r = 0.0;
      for (int k0 = 0; k0 < ycnt; k0 += B) {
        double t[B];
#pragma unroll
        for (int k = 0; k < B; ++k) t[k] = col[(k0 + k < ycnt ? k0 + k : ycnt - 1) * w];
#pragma unroll
        for (int k = 0; k < B; ++k) r += k0 + k < ycnt ? t[k] : 0.0;
      }
      double run, tot;
      stretch_offsets(r, csg, 16, run, tot);
      for (int k0 = 0; k0 < ycnt; k0 += B) {
        double t[B];
#pragma unroll
        for (int k = 0; k < B; ++k) t[k] = col[(k0 + k < ycnt ? k0 + k : ycnt - 1) * w];
#pragma unroll
        for (int k = 0; k < B; ++k) {
          run += k0 + k < ycnt ? t[k] : 0.0;  // (past the end: the last row again, with the same value)
          col[(k0 + k < ycnt ? k0 + k : ycnt - 1) * w] = run;
        }
      }
    }
    __syncthreads();
    SPR_PSTAMP6(8);
    {
      // One float4 per (sub-transform set, pair-kernel lane) = the 1/sigma values of the four pixels that lane weights: every
      // slot is written exactly once, in address order, zeros where no pixel maps to it (inverse of Cfg::inv6_index, as in
      // prep_fft_kernel).  The window of row y is rows [0, y + above) for y <= cy and [y - cy, h) below.
      float4* inv4 = reinterpret_cast<float4*>(item_base + spec_bytes) + static_cast<size_t>(c) * (g.inv_per_chan / 4);
      for (int idx4 = opaque(tid); idx4 < C::kInv6PerChan / 4; idx4 += kPT) {
        const int pp = idx4 / C::NT, lane6 = idx4 - pp * C::NT;
        const int l64 = lane6 & 63, rg = l64 / 3, tq = l64 - 3 * rg;
        const int row = (lane6 >> 6) * C::kRowGroups + rg, n1 = 3 * pp + tq;
        float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (l64 < 63 && n1 < 16 && row < h) {
          const int b = (33 * n1) % 48;
          const int ma = tq == 1 ? b - 32 : b, mb = ma == n1 ? n1 + 16 : n1;
          const bool upper = row <= cy;
          const int hi = upper ? (row + above < h ? row + above : h) - 1 : h - 1;
          const int lo = upper ? 0 : row - cy - 1;
          const double* p1a = H1 + hi * w;
          const double* p1b = H1 + lo * w;
          const double* p2a = H2 + hi * w;
          const double* p2b = H2 + lo * w;
          double a1[4], b1[4], a2[4], b2[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {  // all look-ups of the slot are requested before the first is used
            const int x = 2 * (e < 2 ? ma : mb) + (e & 1), xs = x < w ? x : w - 1;
            a1[e] = p1a[xs]; b1[e] = p1b[xs]; a2[e] = p2a[xs]; b2[e] = p2b[xs];
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int x = 2 * (e < 2 ? ma : mb) + (e & 1);
            const float r = inv_sigma_from_sums(upper ? a1[e] : a1[e] - b1[e], upper ? a2[e] : a2[e] - b2[e], inv_n);
            o[e] = x < w ? r : 0.0f;
          }
        }
        inv4[idx4] = float4{o[0], o[1], o[2], o[3]};
      }
    }
    __syncthreads();  // the row pass writes over the planes
    SPR_PSTAMP6(3);

    // ---- row pass: two real rows per complex transform of length NW (prep_fft_kernel's, scale 1) -------------------
    {
      const int tidv = opaque(tid);
      const int giw = tidv / C::TGW, t = tidv - giw * C::TGW;
      const LdsTwiddles<C::TGW> twr{twt_w, t};
      cf* gbuf = xbuf + giw * C::kRowGroupElems;
      cf* zb = gbuf;
      const int pairs = (h + 1) / 2;
      constexpr int kPairsPerRound = kPT / C::TGW;
      const int rounds = ceil_div(pairs, kPairsPerRound);
      for (int rr = 0; rr < rounds; ++rr) {
        const int pr = rr * kPairsPerRound + giw;
        const int ra = 2 * pr, rb = ra + 1;
        cf x[C::EW], y[GW::SPL][C::TGW];
#pragma unroll
        for (int m = 0; m < C::EW; ++m) {
          const int n2 = GW::in_index(t, m);
          const bool in = n2 < w;
          x[m].x = (in && ra < h) ? x0[ra * w + n2] : 0.0f;
          x[m].y = (in && rb < h) ? x0[rb * w + n2] : 0.0f;
        }
        group_fft<C::EW, C::TGW, -1>(x, y, t, twr, gbuf);
        wave_sync();
#pragma unroll
        for (int pp = 0; pp < GW::SPL; ++pp)
#pragma unroll
          for (int sidx = 0; sidx < C::TGW; ++sidx)
            if (GW::out_valid(t, pp)) zb[GW::out_index(t, pp, sidx)] = y[pp][sidx];
        wave_sync();
        if (pr < pairs) {
          for (int k = t; k <= C::NW / 2; k += C::TGW) {
            const cf zk = zb[k];
            const cf zm = zb[k == 0 ? 0 : C::NW - k];
            F[ra * f_stride + k] = cmake(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
            F[rb * f_stride + k] = cmake(0.5f * (zk.y + zm.y), 0.5f * (zm.x - zk.x));
          }
        }
        wave_sync();
      }
    }
    __syncthreads();
    SPR_PSTAMP6(4);

    // ---- column pass: nw/2 + 1 columns of length NH ------------------------------------------------------------------
    {
      cf* spec = reinterpret_cast<cf*>(item_base) + static_cast<size_t>(c) * C::kSpecPerChan;
      const int tidv = opaque(tid);
      const int gi = tidv / C::TGH, t = tidv - gi * C::TGH;
      const LdsTwiddles<C::TGH> twc{twt_h, t};
      cf* gbuf = xbuf + gi * GH::kGroupElems;
      const int rows_f = 2 * ((h + 1) / 2);
      constexpr int kColsPerRound = kPT / C::TGH;
      constexpr int kRounds = (C::COLS + 1 + kColsPerRound - 1) / kColsPerRound;
      for (int rc = 0; rc < kRounds; ++rc) {
        const int j = rc * kColsPerRound + gi;
        const bool nyq = j == C::COLS;
        const bool active = j <= C::COLS;
        cf x[C::EH], y[GH::SPL][C::TGH];
#pragma unroll
        for (int m = 0; m < C::EH; ++m) {
          const int n1 = GH::in_index(t, m);
          x[m] = (active && n1 < rows_f) ? F[n1 * f_stride + j] : cmake(0.0f, 0.0f);
        }
        group_fft<C::EH, C::TGH, -1>(x, y, t, twc, gbuf);
        if (active) {
#pragma unroll
          for (int pp = 0; pp < GH::SPL; ++pp) {
            if (!GH::out_valid(t, pp)) continue;
#pragma unroll
            for (int sidx = 0; sidx < C::TGH; ++sidx) {
              const int k1 = GH::out_index(t, pp, sidx);
              spec[nyq ? C::kNyqOffset + k1 : C::spec_index(C::slot(j), k1)] = y[pp][sidx];
            }
          }
        }
      }
    }
    __syncthreads();  // F and the exchange buffers are the next channel's planes
    SPR_PSTAMP6(5);
  }
}

}  // namespace

bool prep6_covers(const NccGeom& g) {
  if (!g.six || g.big || !g.prep6) return false;
  if (g.nh != C6::NH || g.nw != C6::NW || g.nt != C6::NT) return false;
  if (g.th < g.ih || g.tw < g.iw) return false;  // corner windows only
  if (g.ih > C6::kRows6 || g.ih * kSeg > kPT || g.iw > 64) return false;
  if (g.ih * g.iw > kLoads * kPT) return false;
  if (g.inv_per_chan != C6::kInv6PerChan) return false;
  return prep6_lds(g).total <= static_cast<size_t>(kLdsLimit);
}

int launch_prep6(const NccGeom& g, const PlanScratch& s, const PrepCall& c) {
  const Prep6Lds l = prep6_lds(g);
  const size_t item_bytes = prepared_gallery_item_bytes(g, SPR_NCC_FFT);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(prep6_gallery_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, kLdsLimit);
  const size_t elem = g.dtype == SPR_F32 ? 4 : 2;
  const size_t raw_item_bytes = static_cast<size_t>(g.channels) * g.g_h * g.g_w * elem;
  const int64_t batch = 65535;  // grid.y
  for (int64_t first = 0; first < c.n; first += batch) {
    const int64_t m = c.n - first < batch ? c.n - first : batch;
    hipLaunchKernelGGL(prep6_gallery_kernel, dim3(ceil_div(g.channels, kChansPerWg), static_cast<unsigned>(m)), dim3(kPT),
                       l.total, c.stream, g,
                       static_cast<const void*>(static_cast<const unsigned char*>(c.maps) + first * raw_item_bytes),
                       static_cast<unsigned char*>(c.prepared) + first * item_bytes, item_bytes, s.tw_h, s.tw_w,
                       static_cast<unsigned>(l.x0_off), static_cast<unsigned>(l.f_off), static_cast<unsigned>(l.xbuf_off),
                       static_cast<unsigned>(l.tw_off), l.f_stride);
    const int rc = check_launch("prep6_gallery_kernel");
    if (rc != SPR_OK) return rc;
  }
  return SPR_OK;
}

#ifdef SPR_PREP6_STAMPS
extern "C" int spr_debug_read_prep_stamps(unsigned long long* host, int n) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_prep6_stamps), sizeof(unsigned long long) * n) == hipSuccess ? 0 : -1;
}
#endif

}  // namespace spr
