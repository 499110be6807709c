// C ABI entry points of libshoeprint_mi355x.so (include/shoeprint_mi355x.h) for the NCC scorer.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <mutex>
#include <new>
#include <vector>

#include "spr_common.h"

namespace spr {

static thread_local char g_error[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
}

int check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return SPR_ERR_HIP;
  }
  return SPR_OK;
}

int env_int(const char* name, int fallback) {
  const char* v = std::getenv(name);
  return v && *v ? std::atoi(v) : fallback;
}

int64_t pair_tiles_per_launch(int pairs_per_tile, int threads) {
  int64_t t = ((static_cast<int64_t>(1) << 32) - 1) / (static_cast<int64_t>(pairs_per_tile) * threads);
  const int64_t by_blocks = ((static_cast<int64_t>(1) << 31) - 1) / pairs_per_tile;
  if (by_blocks < t) t = by_blocks;
  const int cap = env_int("SPR_NCC_MAX_TILES", 0);
  return cap >= 1 && cap < t ? cap : t;
}

size_t prepared_query_item_bytes(const NccGeom& g, int method) {
  size_t b;
  if (method == SPR_NCC_MFMA || method == SPR_NCC_MFMA_F32) return mfma_query_item_bytes(g);
  if (method == SPR_NCC_FFT)
    b = sizeof(cf) * static_cast<size_t>(g.channels) * g.spec_per_chan + static_cast<size_t>(g.channels);  // + dead flags
  else
    b = sizeof(float) * static_cast<size_t>(g.channels) * g.th * g.tw;
  return align_up(b, 256);
}

size_t prepared_gallery_item_bytes(const NccGeom& g, int method) {
  size_t b;
  if (method == SPR_NCC_MFMA || method == SPR_NCC_MFMA_F32) return mfma_gallery_item_bytes(g);
  if (method == SPR_NCC_FFT)
    b = static_cast<size_t>(g.channels) * (sizeof(cf) * g.spec_per_chan + sizeof(float) * g.inv_per_chan) +
        static_cast<size_t>(g.channels);  // + one dead flag per channel
  else
    b = sizeof(float) * static_cast<size_t>(g.channels) * g.ih * g.iw * 2;
  return align_up(b, 256);
}

}  // namespace spr

struct spr_ncc_plan {
  spr::NccGeom geom;
  int method;              // resolved: SPR_NCC_FFT, SPR_NCC_DIRECT, SPR_NCC_MFMA or SPR_NCC_MFMA_F32
  spr::PlanScratch scratch{};
  bool mfma_peaks = false;  // matrix-core plans: spr_ncc_plan_enable_peaks was called (their peak form is opt-in)
  // A plan that owns device scratch its kernels write (the FFT workspace `ws`, the correction matrix `mfma_x`) orders the
  // calls that touch it (PlanCall below); what a plan owns is known when it is created.
  bool owns_scratch = false;
  std::mutex mutex;         // held by the one call that is enqueueing work on the scratch
  hipEvent_t done = nullptr;  // recorded behind that call's launches
  hipStream_t last_stream = nullptr;
  bool used = false;
};

// One call that touches scratch the plan owns, on stream s: host threads take turns, and a call that arrives on ANOTHER
// stream than the last one first waits for that one's launches - two streams sharing a plan (one scorer, equal-shaped layers
// on separate streams) then serialise instead of racing on the scratch.  Nothing at all on a plan that owns none.
class PlanCall {
 public:
  PlanCall(spr_ncc_plan* plan, hipStream_t s) : plan_(plan->owns_scratch ? plan : nullptr), stream_(s) {
    if (!plan_) return;
    plan_->mutex.lock();
    if (!plan_->done && hipEventCreateWithFlags(&plan_->done, hipEventDisableTiming) != hipSuccess) {
      spr::set_error("hipEventCreate failed");
      rc = SPR_ERR_HIP;
    } else if (plan_->used && plan_->last_stream != s && hipStreamWaitEvent(s, plan_->done, 0) != hipSuccess) {
      spr::set_error("hipStreamWaitEvent failed");
      rc = SPR_ERR_HIP;
    }
  }
  ~PlanCall() {
    if (!plan_) return;
    if (rc == SPR_OK) {
      (void)hipEventRecord(plan_->done, stream_);
      plan_->last_stream = stream_;
      plan_->used = true;
    }
    plan_->mutex.unlock();
  }
  PlanCall(const PlanCall&) = delete;
  PlanCall& operator=(const PlanCall&) = delete;
  int rc = SPR_OK;  // not SPR_OK: launch nothing

 private:
  spr_ncc_plan* plan_;
  hipStream_t stream_;
};

using namespace spr;

static int make_twiddles(int n, cf** out) {
  std::vector<cf> host(static_cast<size_t>(n));
  const double two_pi = 6.283185307179586476925286766559;
  for (int k = 0; k < n; ++k) {
    const double a = -two_pi * static_cast<double>(k) / static_cast<double>(n);
    host[k].x = static_cast<float>(std::cos(a));
    host[k].y = static_cast<float>(std::sin(a));
  }
  // exact values on the axes (cos/sin of multiples of pi/2 are not exact in floating point)
  if (n % 4 == 0) {
    host[n / 4] = cf{0.0f, -1.0f};
    host[n / 2] = cf{-1.0f, 0.0f};
    host[3 * n / 4] = cf{0.0f, 1.0f};
  } else if (n % 2 == 0) {
    host[n / 2] = cf{-1.0f, 0.0f};
  }
  void* dev = nullptr;
  if (hipMalloc(&dev, sizeof(cf) * n) != hipSuccess) { set_error("hipMalloc(twiddles) failed"); return SPR_ERR_HIP; }
  if (hipMemcpy(dev, host.data(), sizeof(cf) * n, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(dev);
    set_error("hipMemcpy(twiddles) failed");
    return SPR_ERR_HIP;
  }
  *out = static_cast<cf*>(dev);
  return SPR_OK;
}

extern "C" const char* spr_last_error(void) { return g_error; }
extern "C" int spr_abi_version(void) { return SPR_ABI_VERSION; }

extern "C" int spr_ncc_plan_create(const spr_ncc_shape* shape, spr_ncc_plan** plan_out) {
  if (!shape || !plan_out) { set_error("spr_ncc_plan_create: null pointer"); return SPR_ERR_ARG; }
  *plan_out = nullptr;
  if (shape->channels <= 0 || shape->crop < 0) { set_error("spr_ncc_plan_create: bad channels/crop"); return SPR_ERR_ARG; }
  if (shape->dtype != SPR_F32 && shape->dtype != SPR_F16 && shape->dtype != SPR_BF16) {
    set_error("spr_ncc_plan_create: unknown dtype %d", shape->dtype);
    return SPR_ERR_ARG;
  }
  if (shape->method != SPR_NCC_AUTO && shape->method != SPR_NCC_FFT && shape->method != SPR_NCC_DIRECT &&
      shape->method != SPR_NCC_FFT_POW2 && shape->method != SPR_NCC_MFMA && shape->method != SPR_NCC_MFMA_F32) {
    set_error("spr_ncc_plan_create: unknown method %d", shape->method);
    return SPR_ERR_ARG;
  }
  NccGeom g{};
  g.channels = shape->channels;
  g.q_h = shape->q_h; g.q_w = shape->q_w; g.g_h = shape->g_h; g.g_w = shape->g_w;
  g.crop = shape->crop;
  g.dtype = shape->dtype;
  g.th = g.q_h - 2 * g.crop; g.tw = g.q_w - 2 * g.crop;
  g.ih = g.g_h - 2 * g.crop; g.iw = g.g_w - 2 * g.crop;
  if (g.th < 1 || g.tw < 1 || g.ih < 1 || g.iw < 1) {
    set_error("spr_ncc_plan_create: maps %dx%d / %dx%d vanish under a crop of %d", g.q_h, g.q_w, g.g_h, g.g_w, g.crop);
    return SPR_ERR_SHAPE;
  }
  int method = 0;
  NccGeom gf = g, gd = g;
  const bool fft_ok = fft_geometry(gf, shape->method == SPR_NCC_FFT_POW2), direct_ok = direct_geometry(gd);
  // SPR_NCC_MFMA=0 in the environment keeps SPR_NCC_AUTO off the matrix-core kernel (A/B runs)
  NccGeom gm = g;
  const bool mfma_ok = mfma_geometry(gm), mfma_auto = mfma_ok && env_int("SPR_NCC_MFMA", 1) != 0;
  if (shape->method == SPR_NCC_MFMA) {
    if (!mfma_ok) { set_error("matrix-core method: bfloat16 / float16 maps of 28x12 (cropped) on both sides only, got dtype %d, query %dx%d vs gallery %dx%d", g.dtype, g.th, g.tw, g.ih, g.iw); return SPR_ERR_UNSUPPORTED; }
    method = SPR_NCC_MFMA;
  } else if (shape->method == SPR_NCC_MFMA_F32) {  // asked for by name only: SPR_NCC_AUTO never resolves to it
    gm = g;
    if (!mfma_f32_geometry(gm)) { set_error("float32 matrix-core method: float32 maps, cropped search maps up to 28x12 and cropped templates up to 30x16 only, got dtype %d, query %dx%d vs gallery %dx%d", g.dtype, g.th, g.tw, g.ih, g.iw); return SPR_ERR_UNSUPPORTED; }
    method = SPR_NCC_MFMA_F32;
  } else if (shape->method == SPR_NCC_AUTO && mfma_auto) {
    method = SPR_NCC_MFMA;
  } else if (shape->method == SPR_NCC_FFT || shape->method == SPR_NCC_FFT_POW2) {
    if (!fft_ok) { set_error("FFT method: no instantiated LDS-resident grid fits query %dx%d vs gallery %dx%d", g.th, g.tw, g.ih, g.iw); return SPR_ERR_UNSUPPORTED; }
    method = SPR_NCC_FFT;
  } else if (shape->method == SPR_NCC_DIRECT) {
    if (!direct_ok) { set_error("direct method: maps %dx%d vs %dx%d do not fit LDS", g.th, g.tw, g.ih, g.iw); return SPR_ERR_UNSUPPORTED; }
    method = SPR_NCC_DIRECT;
  } else if (fft_ok) {
    method = SPR_NCC_FFT;
  } else if (direct_ok) {
    method = SPR_NCC_DIRECT;
  } else {
    set_error("no NCC kernel fits query %dx%d vs gallery %dx%d (cropped) in LDS", g.th, g.tw, g.ih, g.iw);
    return SPR_ERR_UNSUPPORTED;
  }
  spr_ncc_plan* p = new (std::nothrow) spr_ncc_plan();
  if (!p) { set_error("out of host memory"); return SPR_ERR_ARG; }
  p->method = method;
  p->geom = method == SPR_NCC_FFT ? gf : (method == SPR_NCC_MFMA || method == SPR_NCC_MFMA_F32) ? gm : gd;
  PlanScratch& sc = p->scratch;
  if (method == SPR_NCC_MFMA && mfma_workspace_bytes(p->geom) > 0 &&
      hipMalloc(reinterpret_cast<void**>(&sc.mfma_x), mfma_workspace_bytes(p->geom)) != hipSuccess) {
    set_error("hipMalloc(%zu bytes of correction matrix) failed", mfma_workspace_bytes(p->geom));
    spr_ncc_plan_destroy(p);
    return SPR_ERR_WORKSPACE;
  }
  if (method == SPR_NCC_FFT) {
    int rc = make_twiddles(p->geom.nh, &sc.tw_h);
    if (rc == SPR_OK) rc = make_twiddles(p->geom.nw, &sc.tw_w);
    const size_t ws_bytes = fft_workspace_bytes(p->geom);
    if (rc == SPR_OK && ws_bytes > 0) {
      if (hipMalloc(&sc.ws, ws_bytes) != hipSuccess) {
        set_error("hipMalloc(%zu bytes of FFT workspace) failed", ws_bytes);
        rc = SPR_ERR_WORKSPACE;
      } else {
        sc.ws_bytes = ws_bytes;
      }
    }
    if (rc == SPR_OK && p->geom.six) {
      // pre-twist factors of the six-wave row pass: cot(pi k / nw + pi / 4), k < nw / 2 (ncc_pair6.hip)
      const int half = p->geom.nw / 2;
      std::vector<float> host(static_cast<size_t>(half));
      for (int k = 0; k < half; ++k) {
        const double x = 3.14159265358979323846 * (static_cast<double>(k) / p->geom.nw + 0.25);
        host[k] = static_cast<float>(std::cos(x) / std::sin(x));
      }
      if (hipMalloc(reinterpret_cast<void**>(&sc.six_ctab), sizeof(float) * half) != hipSuccess ||
          hipMemcpy(sc.six_ctab, host.data(), sizeof(float) * half, hipMemcpyHostToDevice) != hipSuccess) {
        set_error("pre-twist table: hipMalloc / hipMemcpy failed");
        rc = SPR_ERR_HIP;
      }
    }
    if (rc != SPR_OK) { spr_ncc_plan_destroy(p); return rc; }
  }
  p->owns_scratch = sc.mfma_x || sc.ws;
  *plan_out = p;
  return SPR_OK;
}

extern "C" void spr_ncc_plan_destroy(spr_ncc_plan* plan) {
  if (!plan) return;
  const PlanScratch& sc = plan->scratch;
  for (void* dev : std::initializer_list<void*>{sc.tw_h, sc.tw_w, sc.ws, sc.six_ctab, sc.mfma_x})
    if (dev) (void)hipFree(dev);
  if (plan->done) (void)hipEventDestroy(plan->done);
  delete plan;
}

extern "C" int spr_ncc_plan_method(const spr_ncc_plan* plan) { return plan ? plan->method : SPR_ERR_ARG; }

extern "C" int spr_ncc_plan_fft_size(const spr_ncc_plan* plan, int32_t* rows, int32_t* cols) {
  if (!plan || !rows || !cols) { set_error("spr_ncc_plan_fft_size: null pointer"); return SPR_ERR_ARG; }
  *rows = plan->method == SPR_NCC_FFT ? plan->geom.nh : 0;
  *cols = plan->method == SPR_NCC_FFT ? plan->geom.nw : 0;
  return SPR_OK;
}

extern "C" size_t spr_ncc_query_bytes(const spr_ncc_plan* plan, int64_t n) {
  if (!plan || n < 0) return 0;
  return prepared_query_item_bytes(plan->geom, plan->method) * static_cast<size_t>(n);
}
extern "C" size_t spr_ncc_gallery_bytes(const spr_ncc_plan* plan, int64_t n) {
  if (!plan || n < 0) return 0;
  return prepared_gallery_item_bytes(plan->geom, plan->method) * static_cast<size_t>(n);
}

static int prepare(spr_ncc_plan* plan, bool is_query, const void* maps, int64_t n, void* prepared, spr_stream_t stream,
                   const char* who) {
  if (!plan) { set_error("%s: null plan", who); return SPR_ERR_ARG; }
  if (n < 0 || n > 65535) { set_error("%s: n = %lld outside [0, 65535] (call in chunks)", who, static_cast<long long>(n)); return SPR_ERR_ARG; }
  if (n == 0) return SPR_OK;
  if (!maps || !prepared) { set_error("%s: null pointer", who); return SPR_ERR_ARG; }
  const PrepCall c{is_query, maps, n, prepared, static_cast<hipStream_t>(stream)};
  if (plan->method == SPR_NCC_FFT) {
    PlanCall guard(plan, c.stream);  // the workspace-mode prep kernels write scratch.ws (an LDS-resident plan owns nothing)
    return guard.rc != SPR_OK ? guard.rc : launch_prep_fft(plan->geom, plan->scratch, c);
  }
  // (matrix-core preparation does not touch the correction matrix: no guard)
  if (plan->method == SPR_NCC_MFMA || plan->method == SPR_NCC_MFMA_F32) return launch_prep_mfma(plan->geom, plan->scratch, c);
  return launch_prep_direct(plan->geom, plan->scratch, c);
}

extern "C" int spr_ncc_prepare_queries(spr_ncc_plan* plan, const void* maps, int64_t n, void* prepared,
                                       spr_stream_t stream) {
  return prepare(plan, true, maps, n, prepared, stream, "spr_ncc_prepare_queries");
}
extern "C" int spr_ncc_prepare_gallery(spr_ncc_plan* plan, const void* maps, int64_t n, void* prepared,
                                       spr_stream_t stream) {
  return prepare(plan, false, maps, n, prepared, stream, "spr_ncc_prepare_gallery");
}

// the launches of one scoring call
static int score_pairs(spr_ncc_plan* plan, const PairCall& c) {
  PlanCall guard(plan, c.stream);
  if (guard.rc != SPR_OK) return guard.rc;
  if (plan->method == SPR_NCC_FFT) return launch_pair_fft(plan->geom, plan->scratch, c);
  if (plan->method == SPR_NCC_MFMA || plan->method == SPR_NCC_MFMA_F32) return launch_pair_mfma(plan->geom, plan->scratch, c);
  return launch_pair_direct(plan->geom, plan->scratch, c);
}

extern "C" int spr_ncc_score(spr_ncc_plan* plan, const void* pq, int64_t nq, const void* pg, int64_t ng, float* scores,
                             int64_t ld, int64_t col0, int accumulate_max, spr_stream_t stream) {
  if (!plan) { set_error("spr_ncc_score: null plan"); return SPR_ERR_ARG; }
  if (nq < 0 || ng < 0 || col0 < 0 || ld < col0 + ng) { set_error("spr_ncc_score: bad sizes"); return SPR_ERR_ARG; }
  if (nq == 0 || ng == 0) return SPR_OK;
  if (!pq || !pg || !scores) { set_error("spr_ncc_score: null pointer"); return SPR_ERR_ARG; }
  if (nq > 65535 || ng > (1 << 24)) { set_error("spr_ncc_score: too many items in one call (chunk the gallery)"); return SPR_ERR_ARG; }
  return score_pairs(plan, PairCall{pq, nq, pg, ng, scores, ld, col0, accumulate_max, nullptr, static_cast<hipStream_t>(stream)});
}

extern "C" int spr_ncc_plan_has_peaks(const spr_ncc_plan* plan) {
  if (!plan) return 0;
  return plan->method == SPR_NCC_FFT || plan->method == SPR_NCC_DIRECT || plan->mfma_peaks ? 1 : 0;
}

extern "C" int spr_ncc_plan_enable_peaks(spr_ncc_plan* plan) {
  if (!plan) { set_error("spr_ncc_plan_enable_peaks: null plan"); return SPR_ERR_ARG; }
  if (plan->method == SPR_NCC_MFMA || plan->method == SPR_NCC_MFMA_F32) plan->mfma_peaks = true;  // (the others have the form as they are)
  return SPR_OK;
}

extern "C" int spr_ncc_score_peaks(spr_ncc_plan* plan, const void* pq, int64_t nq, const void* pg, int64_t ng, float* scores,
                                   int32_t* peak_yx, int32_t* peak_tag, int64_t ld, int64_t col0, int accumulate_max,
                                   int32_t tag, spr_stream_t stream) {
  if (!plan) { set_error("spr_ncc_score_peaks: null plan"); return SPR_ERR_ARG; }
  if (!spr_ncc_plan_has_peaks(plan)) {  // before anything is launched
    set_error("spr_ncc_score_peaks: the matrix-core methods keep the maximum only (spr_ncc_plan_has_peaks() == 0) unless the "
              "plan was asked with spr_ncc_plan_enable_peaks");
    return SPR_ERR_UNSUPPORTED;
  }
  if (nq < 0 || ng < 0 || col0 < 0 || ld < col0 + ng) { set_error("spr_ncc_score_peaks: bad sizes"); return SPR_ERR_ARG; }
  if (nq == 0 || ng == 0) return SPR_OK;
  if (!pq || !pg || !scores || !peak_yx) { set_error("spr_ncc_score_peaks: null pointer"); return SPR_ERR_ARG; }
  if (nq > 65535 || ng > (1 << 24)) { set_error("spr_ncc_score_peaks: too many items in one call (chunk the gallery)"); return SPR_ERR_ARG; }
  PairCall c{pq, nq, pg, ng, scores, ld, col0, accumulate_max, nullptr, static_cast<hipStream_t>(stream)};
  c.peak_yx = peak_yx;
  c.peak_tag = peak_tag;
  c.tag = tag;
  return score_pairs(plan, c);
}

extern "C" int spr_ncc_plan_has_list(const spr_ncc_plan* plan) {
  if (!plan) return 0;
  return (plan->method == SPR_NCC_FFT && !plan->geom.big) || plan->method == SPR_NCC_DIRECT ? 1 : 0;
}

extern "C" int spr_ncc_score_list(spr_ncc_plan* plan, const void* pq, int64_t nq, const void* pg, int64_t ng,
                                  const int32_t* pairs, int64_t n_pairs, float* scores, int32_t* peak_yx, int32_t* peak_tag,
                                  int accumulate_max, int32_t tag, spr_stream_t stream) {
  if (!plan) { set_error("spr_ncc_score_list: null plan"); return SPR_ERR_ARG; }
  if (!spr_ncc_plan_has_list(plan)) {  // before anything is launched
    set_error("spr_ncc_score_list: the workspace instance of the FFT method and the matrix-core methods have no list form "
              "(spr_ncc_plan_has_list() == 0)");
    return SPR_ERR_UNSUPPORTED;
  }
  if (nq < 0 || ng < 0 || n_pairs < 0) { set_error("spr_ncc_score_list: bad sizes"); return SPR_ERR_ARG; }
  if (n_pairs == 0) return SPR_OK;
  if (!pq || !pg || !pairs || !scores || !peak_yx) { set_error("spr_ncc_score_list: null pointer"); return SPR_ERR_ARG; }
  if (nq > 65535 || ng > (1 << 24)) { set_error("spr_ncc_score_list: too many items in one call (chunk the gallery)"); return SPR_ERR_ARG; }
  PairCall c{pq, nq, pg, ng, scores, n_pairs, 0, accumulate_max, nullptr, static_cast<hipStream_t>(stream)};
  c.peak_yx = peak_yx;
  c.peak_tag = peak_tag;
  c.tag = tag;
  c.pairs = pairs;
  c.n_pairs = n_pairs;
  return score_pairs(plan, c);
}

extern "C" int spr_ncc_plan_has_surfaces(const spr_ncc_plan* plan) { return spr_ncc_plan_has_list(plan); }

extern "C" int spr_ncc_score_surfaces(spr_ncc_plan* plan, const void* pq, int64_t nq, const void* pg, int64_t ng,
                                      const int32_t* pairs, int64_t n_pairs, float* scores, int32_t* peak_yx, int32_t* peak_tag,
                                      float* surfaces, int accumulate_max, int32_t tag, spr_stream_t stream) {
  if (!plan) { set_error("spr_ncc_score_surfaces: null plan"); return SPR_ERR_ARG; }
  if (!spr_ncc_plan_has_surfaces(plan)) {  // before anything is launched
    set_error("spr_ncc_score_surfaces: the workspace instance of the FFT method and the matrix-core methods have no surfaces "
              "form (spr_ncc_plan_has_surfaces() == 0)");
    return SPR_ERR_UNSUPPORTED;
  }
  if (nq < 0 || ng < 0 || n_pairs < 0) { set_error("spr_ncc_score_surfaces: bad sizes"); return SPR_ERR_ARG; }
  if (n_pairs == 0) return SPR_OK;
  if (!pq || !pg || !pairs || !scores || !peak_yx || !surfaces) { set_error("spr_ncc_score_surfaces: null pointer"); return SPR_ERR_ARG; }
  if (nq > 65535 || ng > (1 << 24)) { set_error("spr_ncc_score_surfaces: too many items in one call (chunk the gallery)"); return SPR_ERR_ARG; }
  PairCall c{pq, nq, pg, ng, scores, n_pairs, 0, accumulate_max, nullptr, static_cast<hipStream_t>(stream)};
  c.peak_yx = peak_yx;
  c.peak_tag = peak_tag;
  c.tag = tag;
  c.pairs = pairs;
  c.n_pairs = n_pairs;
  c.surfaces = surfaces;
  return score_pairs(plan, c);
}

extern "C" int spr_ncc_maps(spr_ncc_plan* plan, const void* pq, const void* pg, float* maps_out, spr_stream_t stream) {
  if (!plan || !pq || !pg || !maps_out) { set_error("spr_ncc_maps: null pointer"); return SPR_ERR_ARG; }
  return score_pairs(plan, PairCall{pq, 1, pg, 1, nullptr, 1, 0, 0, maps_out, static_cast<hipStream_t>(stream)});
}
