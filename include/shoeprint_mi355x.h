/*
 * shoeprint_mi355x.h — C ABI of the MI355X-native shoeprint retrieval hot path.
 *
 * The reference (struan-robertson/shoeprint-image-retrieval) is pure Python and has
 * no FFI layer of its own; its hot path is entered through the Python call surface
 * run.py:20-34 uses.  This header is the C-level boundary our host-side mirror of
 * that surface (shoeprint-image-retrieval_amd/similarity.py, network.py) binds with
 * ctypes, and what a maintainer of the reference would bind to replace
 *
 *   similarity.py:26-72    normxcorr            -> spr_ncc_* (per-channel NCC maps)
 *   similarity.py:75-108   get_similarity       -> spr_ncc_score (one pair = Q=G=1)
 *   similarity.py:355-367  score matrix, floor 0, max over variants -> spr_ncc_score
 *   similarity.py:378-386  _get_rank            -> spr_rank_true_match
 *   network.py:185-244     truncated VGG16 forward -> spr_vgg16_* (see below)
 *   network.py:60-71       ToTensor / repeat(3) / Normalize -> fused into the first conv layer
 *
 * (INTEGRATION.md shows the binding stubs.)
 *
 * Conventions
 *  - Every pointer marked "device" is a HIP device pointer owned by the caller
 *    (PyTorch-ROCm allocations in our host code).  Nothing here allocates or frees
 *    caller-visible memory, and nothing synchronises the stream: all work is
 *    enqueued on `stream` (a hipStream_t passed as void*, NULL = default stream).
 *  - All entry points return SPR_OK (0) or a negative error code; spr_last_error()
 *    gives the message for the calling thread.
 *  - Feature maps are dense row-major [item][channel][row][col] ("[N,C,h,w]"),
 *    float32 unless the plan's dtype says otherwise (customtypes.py:7-14,
 *    network.py:241).
 *  - Thread safety: an spr_ncc_plan may be used from several host threads and streams at once (its preparing and scoring
 *    calls; create, enable_peaks and destroy are the owner's).  Every other kind of plan: one host thread at a time.
 *    Different plans are independent.
 *  - An spr_ncc_plan may own device scratch its kernels write: the workspace of the 384 x 192 grid (preparation and
 *    scoring) or the correction matrix of SPR_NCC_MFMA (scoring).  Calls that touch it serialise on the plan: host threads
 *    take turns, and a call arriving on another stream than the last waits for an event recorded behind that one's
 *    launches.  Plans that own nothing (LDS-resident FFT plans, direct plans) pay no lock and no event.  Use one plan per
 *    stream to overlap equal-shaped layers.
 *  - spr_*_plan_create / spr_*_plan_destroy are synchronous (hipMalloc / hipMemcpy / hipFree on the current device): create
 *    plans outside the hot path, with the device that will run them current.
 */
#ifndef SHOEPRINT_MI355X_H
#define SHOEPRINT_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPR_ABI_VERSION 1

enum spr_status {
  SPR_OK = 0,
  SPR_ERR_ARG = -1,         /* null pointer, negative count, bad enum */
  SPR_ERR_SHAPE = -2,       /* shape not representable (e.g. map smaller than the crop) */
  SPR_ERR_UNSUPPORTED = -3, /* valid request this build has no kernel for */
  SPR_ERR_HIP = -4,         /* a HIP runtime call or kernel launch failed */
  SPR_ERR_WORKSPACE = -5    /* caller-provided buffer too small */
};

enum spr_dtype { SPR_F32 = 0, SPR_F16 = 1, SPR_BF16 = 2 };
/* A COMPUTE type of the plain-VGG extractor plans (spr_vgg_plan_create_ex), not a storage type: float32 values split into
 * hi + lo bfloat16, three bf16 matrix-core products per float32 product.  No spr_ncc_* call and no other backbone takes it. */
enum { SPR_COMPUTE_BF16X3 = 3 };

/* Which pair kernel scores a (query, gallery) pair. */
enum spr_ncc_method {
  SPR_NCC_AUTO = 0,   /* bf16 matrix cores when SPR_NCC_MFMA covers the plan, else FFT when an instantiated grid covers the
                         padded maps, else direct */
  SPR_NCC_FFT = 1,    /* frequency-domain correlation, inverse 2-D FFT per channel: LDS-resident for maps up to
                         ~12 k cropped pixels, working set in a plan-owned device workspace beyond that (maps
                         up to 256 x 128 on the 384 x 192 grid); the plan allocates the workspace itself and
                         spr_ncc_plan_create returns SPR_ERR_WORKSPACE if that allocation fails */
  SPR_NCC_DIRECT = 2, /* sliding-window correlation in LDS (any shape that fits LDS) */
  SPR_NCC_FFT_POW2 = 3, /* as SPR_NCC_FFT but restricted to power-of-two grids (A/B and fallback for the 3*2^k grids) */
  SPR_NCC_MFMA = 4,   /* sliding-window correlation as a [queries x taps] x [taps x positions] product on the bf16 / f16 matrix
                         cores: bfloat16 or float16 storage, cropped search maps up to 28 x 12 and cropped templates up to
                         30 x 16 (ResNet50 layer3 / VGG16 conv5_3 / EfficientNet stride-16 maps of a 512 x 256 image and their
                         scaled / rotated query variants; 28 x 12 on both sides has its own tuned instance);
                         SPR_ERR_UNSUPPORTED for anything else */
  SPR_NCC_MFMA_F32 = 5 /* the same product for FLOAT32 storage: both maps are centred in float32 and
                         split into two bfloat16 numbers each (hi + lo), three bf16 matrix-core products per step
                         (hi*hi + hi*lo + lo*hi, f32 accumulation).  Accuracy: 2^-17 per operand - scores within 5e-6 of the
                         float64 oracle where many taps and channels average that out (multi-channel maps under templates of
                         28 x 12 taps and more), measured up to 6.1e-6 per pixel under 3 x 3 taps; the contract is 1e-4.
                         Same shape bounds as SPR_NCC_MFMA, SPR_ERR_UNSUPPORTED for
                         other storage types or shapes.  Chosen by name only: SPR_NCC_AUTO never resolves to it */
};

typedef void* spr_stream_t;
typedef struct spr_ncc_plan spr_ncc_plan;

const char* spr_last_error(void);
int spr_abi_version(void);

/* ------------------------------------------------------------------ NCC scorer
 *
 * A plan fixes one (query shape, gallery shape) class: all queries are
 * [C, q_h, q_w], all gallery items [C, g_h, g_w] (raw sizes, before the crop of
 * `crop` pixels per edge that get_similarity applies, similarity.py:92-93; the
 * reference uses crop = 2).  Ragged data sets are handled by the host code with one
 * plan per shape class.
 */
typedef struct spr_ncc_shape {
  int32_t channels;
  int32_t q_h, q_w;
  int32_t g_h, g_w;
  int32_t crop;
  int32_t dtype;   /* spr_dtype of the feature maps handed to spr_ncc_prepare_* */
  int32_t method;  /* spr_ncc_method */
} spr_ncc_shape;

int spr_ncc_plan_create(const spr_ncc_shape* shape, spr_ncc_plan** plan_out);
void spr_ncc_plan_destroy(spr_ncc_plan* plan);
/* The method the plan resolved to: SPR_NCC_FFT / SPR_NCC_DIRECT / SPR_NCC_MFMA for SPR_NCC_AUTO, or SPR_NCC_MFMA_F32. */
int spr_ncc_plan_method(const spr_ncc_plan* plan);
/* FFT grid the plan uses ({0,0} for the direct method): rows, cols. */
int spr_ncc_plan_fft_size(const spr_ncc_plan* plan, int32_t* rows, int32_t* cols);

/* Bytes of device memory the prepared form of n items needs. */
size_t spr_ncc_query_bytes(const spr_ncc_plan* plan, int64_t n_queries);
size_t spr_ncc_gallery_bytes(const spr_ncc_plan* plan, int64_t n_gallery);

/* Prepare n items (device, [n,C,h,w]) into `prepared` (device, >= *_bytes(n)):
 *  queries  (templates): crop, subtract the per-channel mean (similarity.py:48), scale by
 *           1/sqrt(sum t0^2) (:67-68), and for the FFT method transform to the frequency
 *           domain with the 'same'-mode centre shift (h//2, w//2) folded in.
 *  gallery  (search images): crop, subtract the per-channel mean (:49), float64 window
 *           sums -> 1/sqrt(var) map with var<=0 -> 0 (:57-65, :70), and for the FFT method
 *           the forward transform of the zero-padded map. */
int spr_ncc_prepare_queries(spr_ncc_plan* plan, const void* maps, int64_t n, void* prepared,
                            spr_stream_t stream);
int spr_ncc_prepare_gallery(spr_ncc_plan* plan, const void* maps, int64_t n, void* prepared,
                            spr_stream_t stream);

/* scores[q*ld + col0 + g] = max(prev, get_similarity(query q, gallery g)) as float32, where
 * prev is 0 when accumulate_max == 0 (the reference's zero-initialised matrix,
 * similarity.py:355) and the value already stored otherwise (max over rotation/scale
 * variants, :364-367).  scores: device float32 [n_queries, ld]. */
int spr_ncc_score(spr_ncc_plan* plan, const void* prepared_queries, int64_t n_queries,
                  const void* prepared_gallery, int64_t n_gallery, float* scores, int64_t ld,
                  int64_t col0, int accumulate_max, spr_stream_t stream);

/* spr_ncc_score with the position of every pair's maximum, out of the same pass (the arg-max is kept beside the max in the
 * pair kernels' epilogue; nothing is added to their channel loop).  peak_yx / peak_tag: device int32 [n_queries, ld], indexed
 * exactly like scores (same ld and col0); peak_tag may be NULL.
 *  - scores receives bit for bit what spr_ncc_score writes for the same arguments.
 *  - Let s be the pair's score (floored at 0 as ever) and p = (y << 16) | x the position of the maximum of the channel-summed
 *    map, in cropped search-map coordinates (the convention of spr_maps_peak: the cropped template's top-left corner lies at
 *    (y - th/2, x - tw/2)).  Among equal float32 sums the first position in row-major order wins; the reduction orders
 *    (value, position) pairs, so the result does not depend on lane, wave or work-item order.  The sums are the kernels'
 *    float32 channel sums, while spr_maps_peak adds the per-channel maps in float64: the two may name different pixels where
 *    the two largest sums lie within rounding of each other.
 *  - accumulate_max == 0: the entry becomes (s, p, tag) if s > 0, else (0, -1, -1).
 *  - accumulate_max != 0: the entry is replaced by (s, p, tag) if s > prev, or if s == prev, s > 0 and tag < prev_tag (a
 *    caller that walks variants in another order than their numbers still ends with the lowest number among equal scores);
 *    otherwise it is left alone.  The caller starts the three matrices at 0 / -1 / -1.  The stored tag is read and compared
 *    only when peak_tag is given.
 *  - Limits and launch slicing as for spr_ncc_score.  spr_ncc_plan_has_peaks: 1 for SPR_NCC_FFT and SPR_NCC_DIRECT plans.
 *    A plan of the matrix-core methods (SPR_NCC_MFMA, SPR_NCC_MFMA_F32) answers 0 unless it was asked for the peak form with
 *    spr_ncc_plan_enable_peaks (below): by default its kernels keep the maximum only, spr_ncc_score_peaks returns
 *    SPR_ERR_UNSUPPORTED on it and launches nothing (locate those pairs with spr_ncc_maps + spr_maps_peak).  spr_ncc_score
 *    and spr_ncc_maps are unchanged, on every plan, asked or not. */
int spr_ncc_plan_has_peaks(const spr_ncc_plan* plan); /* 1 / 0 */
/* Ask the plan for the peak form.  SPR_OK on every plan; a no-op on FFT / direct plans.  Afterwards
 * spr_ncc_plan_has_peaks(plan) == 1 and spr_ncc_score_peaks works on it, by the contract written above
 * spr_ncc_score_peaks word for word (scores bit for bit those of spr_ncc_score, first maximum of the
 * kernel's float32 channel sums in row-major order, accumulate / tag rule, limits).  A matrix-core plan takes the arg-max
 * behind its channel loop in all four forms (bfloat16 exact - after the correction matrix is subtracted -, bfloat16 hi + lo,
 * float16, float32 hi + lo) and names positions of the cropped search map only, never a spare position of its 28 x 12
 * frame.  Prepared layouts and sizes do not depend on the call.  SPR_ERR_ARG for a NULL plan. */
int spr_ncc_plan_enable_peaks(spr_ncc_plan* plan);
int spr_ncc_score_peaks(spr_ncc_plan* plan, const void* prepared_queries, int64_t n_queries,
                        const void* prepared_gallery, int64_t n_gallery, float* scores, int32_t* peak_yx,
                        int32_t* peak_tag, int64_t ld, int64_t col0, int accumulate_max, int32_t tag,
                        spr_stream_t stream);

/* The list form of spr_ncc_score_peaks: a list of pairs instead of the whole n_queries x n_gallery grid (the second stage of
 * a coarse-to-fine retrieval scores a few candidates per query on an expensive layer).  pairs: device int32 [n_pairs][2] of
 * (position in prepared_queries, position in prepared_gallery); scores, peak_yx: device arrays of n_pairs entries, and so is
 * peak_tag unless it is NULL.  It is a peak form always: lists are thousands of pairs, not millions.
 *  - Entry p receives bit for bit what spr_ncc_score_peaks stores in cell (q, g) = pairs[p] for the same plan, prepared
 *    buffers, accumulate_max, tag and previous entry: the score floored at 0, the first maximum in row-major order,
 *    (0, -1, -1) where the score is 0, and the accumulate / tag rule written above.
 *  - Pairs may repeat and come in any order; every entry has its own output, so no two workgroups write the same word.
 *    (Neighbouring entries that name the same gallery item share its lines in L2: a caller that can sorts by g.)
 *  - An entry whose q lies outside [0, n_queries) or whose g lies outside [0, n_gallery) is skipped: nothing is read for it
 *    and its three outputs are left alone.  The list is device data the host cannot look at, so the kernels test every entry;
 *    it is also how a caller pads a list.
 *  - n_pairs == 0 is a no-op.  A NULL pointer (peak_tag excepted) or a negative size is SPR_ERR_ARG; n_queries and n_gallery
 *    have the limits of spr_ncc_score.  Launches are sliced as the dense forms' are, so n_pairs has no limit of its own.
 *  - spr_ncc_plan_has_list: 1 for SPR_NCC_FFT plans whose working set lies in LDS (every grid but the 384 x 192 workspace
 *    instance) and for SPR_NCC_DIRECT plans; 0 for the workspace instance, whose kernel is a persistent team grid, and for
 *    the matrix-core methods, whose workgroups score 64 queries per gallery item.  On those spr_ncc_score_list returns
 *    SPR_ERR_UNSUPPORTED before anything is launched (score the block densely and gather the cells). */
int spr_ncc_plan_has_list(const spr_ncc_plan* plan); /* 1 / 0 */
int spr_ncc_score_list(spr_ncc_plan* plan, const void* prepared_queries, int64_t n_queries,
                       const void* prepared_gallery, int64_t n_gallery, const int32_t* pairs, int64_t n_pairs,
                       float* scores, int32_t* peak_yx, int32_t* peak_tag, int accumulate_max, int32_t tag,
                       spr_stream_t stream);

/* The list form that also stores every pair's correlation surface: the channel-mean NCC map an examiner judges a peak by
 * (is it sharp and alone, or one ripple of a periodic tread pattern; is a second alignment almost as good).  The pair kernels
 * hold the finished map in registers in their epilogue; this form stores it instead of discarding it.  surfaces: device
 * float32 [n_pairs][ih][iw], ih x iw = (g_h - 2 crop) x (g_w - 2 crop), the map shape of spr_ncc_maps; it does not depend on
 * the template ('same' mode), so one buffer serves all variants of a query.
 *  - scores, peak_yx, peak_tag receive bit for bit what spr_ncc_score_list stores for the same arguments and previous entries.
 *  - surfaces[p][y][x] = acc(y, x) / (float)channels, where acc is the kernel's own float32 channel sum - the value the
 *    arg-max is taken on -, not floored; the division is the float32 division that gives the score.  Hence
 *    max(max over the surface, 0) has the bits of the entry's new score, and where the score is positive the surface at
 *    peak_yx holds its maximum.  (The peak need not be the FIRST row-major arg-max of the surface: two sums may round to one
 *    quotient.)
 *  - accumulate_max == 0: the surface of every live entry is written, all ih * iw pixels, also where the score is 0.
 *  - accumulate_max != 0: the surface is written if and only if this call replaces the entry's (score, peak, tag) by the rule
 *    written above spr_ncc_score_peaks; otherwise all of it is left alone.  After a walk over variants the buffer holds the
 *    winning variant's map.
 *  - An entry that names no item is skipped: its four outputs are untouched.  Pairs may repeat.  n_pairs == 0 is a no-op.
 *  - A NULL surfaces is SPR_ERR_ARG; the other argument checks, the limits and the launch slicing are spr_ncc_score_list's.
 *  - spr_ncc_plan_has_surfaces: 1 exactly where spr_ncc_plan_has_list is 1.  On the workspace instance and the matrix-core
 *    methods the call returns SPR_ERR_UNSUPPORTED before anything is launched (take spr_ncc_maps + spr_maps_mean there). */
int spr_ncc_plan_has_surfaces(const spr_ncc_plan* plan); /* 1 / 0 */
int spr_ncc_score_surfaces(spr_ncc_plan* plan, const void* prepared_queries, int64_t n_queries,
                           const void* prepared_gallery, int64_t n_gallery, const int32_t* pairs, int64_t n_pairs,
                           float* scores, int32_t* peak_yx, int32_t* peak_tag, float* surfaces, int accumulate_max,
                           int32_t tag, spr_stream_t stream);

/* Debug / parity entry point (scripts/summed_feature_maps.py:1-6, similarity.py:100-104):
 * per-channel NCC maps of ONE prepared query against ONE prepared gallery item, float32
 * [C, g_h-2*crop, g_w-2*crop] (device). */
int spr_ncc_maps(spr_ncc_plan* plan, const void* prepared_query, const void* prepared_gallery,
                 float* maps_out, spr_stream_t stream);

/* ------------------------------------------------------------------ ranking
 * ranks[q] = 1-based position of gallery item match[q] in the descending order of row q
 * (similarity.py:378-386): 1 + #{s_j > s_m} + #{j > m : s_j == s_m} (ties as a stable
 * argsort + flip orders them).  A match index outside [0, n_gallery) gives rank 0 and the
 * call returns SPR_OK; the host mirror turns that into the reference's IndexError.
 * scores: device float32 [n_queries, ld]; match, ranks: device int32 [n_queries]. */
int spr_rank_true_match(const float* scores, int64_t ld, int64_t n_queries, int64_t n_gallery,
                        const int32_t* match, int32_t* ranks, spr_stream_t stream);

/* Partial form for a gallery sharded over ranks: counts[q] = #{j in this shard : s_j > s_m}
 * + #{j in this shard, global index > m : s_j == s_m}, given the true-match score of every
 * query (match_scores, device float32 [n_queries]) and the global index of local column 0.
 * Summing counts over shards and adding 1 gives the rank. */
int spr_rank_count_greater(const float* scores, int64_t ld, int64_t n_queries, int64_t n_local,
                           int64_t global_col0, const float* match_scores, const int32_t* match,
                           int32_t* counts, spr_stream_t stream);

/* dst[i] = keep * dst[i] + weight * src[i] over n float32 score-matrix elements (keep = 0: dst is only written).
 * The reference scores ONE feature layer (run.py:20); a multi-layer score (BASELINE config 5: mean of the conv3_3,
 * conv4_3 and conv5_3 similarities, build-defined) is fused with this on the device. */
int spr_scores_fuse(float* dst, const float* src, int64_t n, float keep, float weight, spr_stream_t stream);

/* ------------------------------------------------------------------ shortlist: top-k and peak localisation
 * spr_topk_rows: for every query row the k best items in the ranker's order - item a before item b iff s_a > s_b, or
 * s_a == s_b (the float ==: -0.0 and +0.0 tie) and idx_a > idx_b - so the item written at position p (1-based) is the item
 * spr_rank_true_match ranks p.  scores: device float32 [n_queries, ld], of which columns [0, n_cols) are read.  The item
 * index of column j is global_col0 + j when col_index is NULL (a shard of a gallery: the global index of local column 0);
 * otherwise it is col_index[q*ld + j] (device int32 [n_queries, ld]) and columns whose entry is negative (-1) are skipped:
 * that form merges candidate lists gathered from shards.  No index may occur twice in a row.  out_scores / out_index:
 * device float32 / int32 [n_queries, k]; positions beyond the number of items hold score 0 and index -1 (n_cols == 0:
 * all of them).  1 <= k <= 256 and item indices below 2^31, else SPR_ERR_ARG; scores are finite by contract
 * (spr_ncc_score stores 0 for non-finite values).  The result does not depend on the grid: any n_queries works. */
int spr_topk_rows(const float* scores, int64_t ld, int64_t n_queries, int64_t n_cols, const int32_t* col_index,
                  int64_t global_col0, int32_t k, float* out_scores, int32_t* out_index, spr_stream_t stream);

/* spr_maps_peak: for every pair p the peak of its channel-summed NCC maps and where it is.  maps: device float32
 * [n_pairs, channels, h, w] (what spr_ncc_maps writes, pair after pair).  acc(y, x) = sum over c of (double)maps[p][c][y][x],
 * added sequentially for c = 0, 1, ... starting from 0.0 (a fixed order: the result is bit-reproducible); the peak is the
 * first maximum of acc in row-major order (numpy's argmax); out_score[p] = (float)(max / channels) - get_similarity's value,
 * similarity.py:100-108, without the floor at 0 - and out_yx[2p], out_yx[2p + 1] = its row and column in cropped search-map
 * coordinates: the cropped template's top-left corner lies at (y - th/2, x - tw/2).  An all-zero map gives score 0 at (0, 0).
 * channels, h, w >= 1, else SPR_ERR_ARG; n_pairs == 0 is a no-op. */
int spr_maps_peak(const float* maps, int64_t n_pairs, int32_t channels, int32_t h, int32_t w, float* out_score,
                  int32_t* out_yx, spr_stream_t stream);

/* spr_maps_mean: the channel-mean map of every pair, for plans without a surfaces form.  maps as for spr_maps_peak;
 * out: device float32 [n_pairs, h, w], out[p][y][x] = (float)(acc(y, x) / channels) with spr_maps_peak's float64 acc
 * (sequential over c, starting from 0.0), so the maximum of out[p] has the bits of spr_maps_peak's out_score[p].
 * channels, h, w >= 1, else SPR_ERR_ARG; n_pairs == 0 is a no-op. */
int spr_maps_mean(const float* maps, int64_t n_pairs, int32_t channels, int32_t h, int32_t w, float* out,
                  spr_stream_t stream);

/* spr_surface_peaks: the n_peaks best separated peaks of every surface and the peak-to-sidelobe ratio of the first.
 * surfaces: device float32 [n, h, w] (spr_ncc_score_surfaces, spr_maps_mean; finite values).  out_value: device float32
 * [n, n_peaks]; out_yx: device int32 [n, n_peaks], positions packed as (y << 16) | x; out_psr: device float32 [n] or NULL.
 *  - Peak 0 is the maximum: the larger value, among equal values the first in row-major order; its sign does not matter.
 *  - Peak j is the same maximum over the pixels outside every window |y - y_i| <= ry && |x - x_i| <= rx of the peaks i < j.
 *    Slots for which no pixel is left hold value 0 and position -1.  Values and positions are exact.
 *  - out_psr = (float)((v0 - mu) / sigma), mu and sigma^2 the mean and the population variance of the pixels outside peak
 *    0's window, accumulated in float64 in two passes (mu, then the sum of (v - mu)^2); 0 when fewer than two such pixels
 *    exist or sigma is 0.
 *  - SPR_ERR_ARG unless 1 <= n_peaks <= 8, ry >= 0, rx >= 0 and 1 <= h, w <= 32767; n == 0 is a no-op. */
int spr_surface_peaks(const float* surfaces, int64_t n, int32_t h, int32_t w, int32_t n_peaks, int32_t ry, int32_t rx,
                      float* out_value, int32_t* out_yx, float* out_psr, spr_stream_t stream);

/* ------------------------------------------------------------------ device-resident ragged sets (features.py)
 * spr_items_gather: item k of dst (k < n) is item index[k] of src, converted to dst_dtype (an spr_dtype).  src: device
 * float32 [*, item_elems], dense; index: DEVICE int32 [n], may repeat, any order, every value a valid item of src (not
 * checked: the caller owns it); dst: device [n, item_elems] of dst_dtype, dense.  The conversion rounds to nearest even:
 * on finite inputs the bits are those of torch's .to(float16 / bfloat16); +-inf pass through, float16 overflow gives inf,
 * -0 is kept, NaN stays NaN (float32 -> float32 copies the bits; a 16-bit NaN's payload is unspecified).  src is only
 * read, nothing outside [dst, dst + n * item_elems * size) is written.  item_elems need not be a multiple of 4; every
 * offset is 64-bit (a shape class may exceed 4 GiB) and the grid strides over the items, so n has no limit of its own.
 * src must be 4-byte aligned and dst aligned to its element size, sizes >= 0 and dst_dtype known, else SPR_ERR_ARG;
 * n == 0 or item_elems == 0 is a no-op.  This is the upload + cast of one shape class or gallery chunk in one pass. */
int spr_items_gather(const float* src, int64_t item_elems, const int32_t* index, int64_t n, void* dst, int32_t dst_dtype,
                     spr_stream_t stream);

/* spr_block_scatter: dst[rows[i] * ld + cols[j]] <- src[i * src_ld + j] for i < nr, j < nc, on 4-byte elements.
 * mode 0 copies the bits (int32 position / variant matrices); mode 1 stores the float32 maximum of the two (a score
 * matrix; the entry is left alone unless src is greater, so scores given to accumulate into survive).  rows / cols: DEVICE
 * int32 [nr] / [nc].  PRECONDITION: the values of rows are distinct and those of cols are distinct, rows[i] * ld + cols[j]
 * lies inside dst - the kernel cannot check device-side contents, its callers guarantee them.  dst and src must not
 * overlap.  nr, nc >= 0, mode 0 | 1, ld >= nc and src_ld >= nc, else SPR_ERR_ARG; nr == 0 or nc == 0 is a no-op. */
int spr_block_scatter(void* dst, int64_t ld, const void* src, int64_t src_ld, const int32_t* rows, int64_t nr,
                      const int32_t* cols, int64_t nc, int32_t mode, spr_stream_t stream);

/* ------------------------------------------------------------------ query variants (rotation / scale)
 * similarity.py:230-284 pushes every query feature map through Pillow: Image.rotate(angle) (NEAREST, no
 * expand, zero fill) or Image.resize((int(w*s), int(h*s))) (BICUBIC on mode "F").  These two entry
 * points restate Pillow's C paths bit for bit; the small parameter sets are computed by the host
 * (shoeprint-image-retrieval_amd/variants.py).  in/out: device float32 [n_maps, h, w] -> [n_maps, h', w'].
 *
 * spr_rotate_nearest: mode 0 copy (0 deg), 1 exact flip (180 deg), 2 / 3 exact 90 / 270 transposes (square
 *   maps), 4 Pillow's 16.16 fixed-point affine walk with fixed6 = {a0,a1,a2,a3,a4,a5} (host array).
 * spr_resample_axis: one pass of Pillow's separable resampler along axis 1 (width) or 0 (height):
 *   bounds = device int32 [out_size][2] (first source index, count), coeffs = device float64
 *   [out_size][ksize] (normalised weights), double accumulation, float32 result. */
int spr_rotate_nearest(const float* in, float* out, int64_t n_maps, int32_t h, int32_t w, int32_t mode,
                       const int64_t* fixed6, spr_stream_t stream);
int spr_resample_axis(const float* in, float* out, int64_t n_maps, int32_t h, int32_t w, int32_t axis,
                      int32_t out_size, const int32_t* bounds, const double* coeffs, int32_t ksize,
                      spr_stream_t stream);

/* ------------------------------------------------------------------ image crop + resize (8-bit LANCZOS)
 * dataloader.py:217-237 loads every image as image.crop(box).resize((int(w*scale), int(h*scale)), LANCZOS).  This entry point
 * restates the 8-bit path of Pillow's separable resampler (Resample.c) bit for bit on a ragged batch of decoded images of one
 * mode: channels = 1 (mode "L", [h, w]) or 3 (mode "RGB", [h, w, 3] interleaved).  Horizontal pass first, its result clamped
 * to 8 bits in the workspace, then the vertical pass; a pass whose size does not change is skipped, an item neither of whose
 * sizes changes is copied.  The crop box is only addressing: no cropped copy is made.
 *
 * A table of one axis for one (source size, output size) pair is int32: [out][2] (first source index, tap count) followed by
 * [out][ksize] coefficients in 22-bit fixed point, each in [-2^23, 2^23) (image_resize.py: lanczos_tables).  Per output sample
 * acc = (1 << 21) + sum(pixel * k) in wrapping 32-bit arithmetic, result = clamp(acc >> 22, 0, 255) (arithmetic shift).
 * The source size of the horizontal table is box_w, of the vertical table box_h; items may share tables.
 *
 * spr_image_resize_layout (host only, no device work): checks every item of the HOST array, fills in its `filled by the
 * layout` members, and returns the workspace size (may be 0) and the two launch sizes that spr_image_resize_u8 takes.  An item
 * with an output size below 1, a box outside the image, or a table on a pass that keeps its size (or none on one that does
 * not) gives SPR_ERR_ARG.  n == 0 is valid.
 * spr_image_resize_u8: in / out / tables / workspace and the array of n laid-out items are DEVICE memory, `blocks` the two
 * host integers of the layout; offsets of an item are bytes from `in` and `out`, its table offsets count int32 from `tables`.
 * Two launches whatever n is.  in, out and the workspace may not overlap; the workspace pointer must not be null even where
 * its size is 0.  n == 0 launches nothing. */
typedef struct spr_image_resize_item {
  int64_t in_off;    /* bytes from `in` to the first pixel of the decoded image */
  int64_t out_off;   /* bytes from `out` to the result, dense [out_h, out_w, channels] */
  int64_t tmp_off;   /* filled by the layout: the item's horizontal result in the workspace */
  int32_t in_h, in_w, in_stride;          /* decoded image; row stride in bytes */
  int32_t box_x, box_y, box_w, box_h;     /* crop box inside it */
  int32_t out_w, out_h;
  int32_t htab, vtab;                     /* offset of the axis' table, -1 where box_w == out_w / box_h == out_h */
  int32_t hk, vk;                         /* ksize of each table */
  int32_t tmp_stride, hblock0, vblock0;   /* filled by the layout */
} spr_image_resize_item;
int spr_image_resize_layout(spr_image_resize_item* items, int64_t n, int32_t channels, size_t* workspace_bytes,
                            int32_t* blocks);
int spr_image_resize_u8(const uint8_t* in, uint8_t* out, const spr_image_resize_item* items, int64_t n, int32_t channels,
                        const int32_t* tables, const int32_t* blocks, void* workspace, spr_stream_t stream);

/* ------------------------------------------------------------------ feature extractor (VGG16)
 *
 * network.py:125-134, 185-186: torchvision vgg16().features truncated to its first `block` children
 * (index -> layer: 0 conv1_1 1 ReLU 2 conv1_2 3 ReLU 4 pool | 5 conv2_1 6 R 7 conv2_2 8 R 9 pool |
 * 10 conv3_1 11 R 12 conv3_2 13 R 14 conv3_3 15 R 16 pool | 17 conv4_1 .. 22 R 23 pool | 24 conv5_1 .. 29 R
 * 30 pool), convolutions 3x3 / stride 1 / zero pad 1 / bias, pools 2x2 stride 2 (floor).  Every
 * convolution runs as an implicit GEMM on the fp32 matrix cores (v_mfma_f32_16x16x4_f32: exact f32
 * fma chains) with bias, ReLU and the following pool fused into its epilogue.
 *
 * Pre-processing fused into the first layer (network.py:60-71, 127-130): x'_c = (pixel/255 - mean_c)/std_c
 * with the zero padding applied AFTER normalisation.  `mean`/`inv_std` are the three per-channel values in
 * [0,1] units (VGG16: mean (0.48235, 0.45882, 0.40784), std 1/255 each).  CLAHE (network.py:197-208) is
 * a separate entry point (spr_clahe_u8) the caller runs before this one.
 */
/* CLAHE of n uint8 images [n, h, w] (device), OpenCV's 8-bit algorithm: tile grid tiles_x x tiles_y
 * (cv2 tileGridSize = (x, y)), clip limit as in cv2.createCLAHE.  workspace: device buffer of
 * spr_clahe_workspace_bytes() (the per-tile look-up tables).  in and out may not alias. */
size_t spr_clahe_workspace_bytes(int64_t n, int32_t tiles_x, int32_t tiles_y);
int spr_clahe_u8(const uint8_t* in, uint8_t* out, int64_t n, int32_t h, int32_t w, float clip_limit,
                 int32_t tiles_x, int32_t tiles_y, void* workspace, spr_stream_t stream);

typedef struct spr_vgg16_plan spr_vgg16_plan;

/* Plain-VGG backbones of network.py:121-139: the truncation model.features[:block] of torchvision's vgg16
 * (cfg "D"), vgg19 (cfg "E") or vgg19_bn.  The plan type keeps its first name; spr_vgg16_plan_create(block)
 * is spr_vgg_plan_create(SPR_VGG16, block).  BatchNorm2d (eval mode) is folded into the preceding
 * convolution's weights and bias by the caller when spr_vgg_conv_info reports it inside the truncation. */
typedef enum spr_vgg_arch { SPR_VGG16 = 0, SPR_VGG19 = 1, SPR_VGG19_BN = 2 } spr_vgg_arch;
int spr_vgg_plan_create(int32_t arch, int32_t block, spr_vgg16_plan** plan_out);
/* As spr_vgg_plan_create with a compute type for the convolutions: SPR_F32 = the f32 matrix cores
 * (exact, the reference's arithmetic: network.py:235 runs the model in float32), SPR_F16 / SPR_BF16 = 16-bit operands with
 * f32 accumulation on v_mfma_f32_16x16x32_{f16,bf16} (BASELINE configs 3 and 5 ask for reduced precision): the weights and
 * the activations BETWEEN layers (and the normalised image the first convolution reads) are rounded to that type (nearest even),
 * bias / ReLU / pool and the last layer's output stay f32; a plan that consists of the first convolution alone stays f32.  Every later call on the plan (packed bytes, pack, workspace, forward)
 * follows the plan's type; the float32 NCHW output and the argument lists do not change.
 *
 * SPR_COMPUTE_BF16X3: float32-grade arithmetic on the bf16 matrix cores (conv_x3_kernel).  The contract:
 *   split(v), v float32:  hi = round_bf16(v) (nearest even), lo = round_bf16(v - float(hi)); the subtraction is exact in
 *                         float32, and v^ = float(hi) + float(lo) is exact in float32 and equals v to <= 2^-16 |v|.
 *   weights               of every convolution behind the first are split once by spr_vgg16_pack_weights; the bias stays
 *                         float32; the first convolution keeps its float32 layout and its float32 fmaf arithmetic (K = 27).
 *   every later conv      per 32-channel chunk and tap three v_mfma_f32_16x16x32_bf16 into the same float32 accumulators, in
 *                         this order: a_hi w_hi, a_hi w_lo, a_lo w_hi (a_lo w_lo, <= 2^-16 |a||w|, is dropped); chunks
 *                         ascending, the nine taps ascending inside a chunk.
 *   epilogue              + bias, ReLU, the float32 NCHW feature tap, the fused 2x2 max pool; the last stage stores float32
 *                         NCHW `out`, every other stage (the first convolution included) stores split(value).
 *   stored activations    NHWC, 4 bytes per channel (packed bytes, workspace and trace sizes are the float32 plan's): per pixel
 *                         and per chunk of 32 channels 64 uint16 words - the 32 hi bfloat16 bit patterns of channels
 *                         32 k .. 32 k + 31, then their 32 lo patterns; word index of (pixel p, channel c, part) =
 *                         (p * C / 32 + c / 32) * 64 + part * 32 + c % 32 with part 0 = hi, 1 = lo.
 * A plan that is its first convolution alone runs in float32, as for the 16-bit types.  spr_resnet_plan_create_ex,
 * spr_effnet_plan_create_ex and spr_densenet_plan_create_ex answer SPR_ERR_UNSUPPORTED to this type (null plan). */
int spr_vgg_plan_create_ex(int32_t arch, int32_t block, int32_t compute, spr_vgg16_plan** plan_out);
int spr_vgg_plan_compute(const spr_vgg16_plan* plan);
/* For convolution conv_index: its position in model.features (state-dict key features.<k>.weight) and whether
 * the BatchNorm2d that follows it (features.<k+1>) lies inside features[:block]. */
int spr_vgg_conv_info(const spr_vgg16_plan* plan, int32_t conv_index, int32_t* feature_index, int32_t* bn_inside);
int spr_vgg16_plan_create(int32_t block, spr_vgg16_plan** plan_out);
void spr_vgg16_plan_destroy(spr_vgg16_plan* plan);
/* Number of convolution layers inside features[:block] and their (cin, cout). */
int spr_vgg16_num_convs(const spr_vgg16_plan* plan);
int spr_vgg16_conv_shape(const spr_vgg16_plan* plan, int32_t conv_index, int32_t* cin, int32_t* cout);
/* Output shape [channels, h, w] for an in_h x in_w image. */
int spr_vgg16_output_shape(const spr_vgg16_plan* plan, int32_t in_h, int32_t in_w, int32_t* channels,
                           int32_t* out_h, int32_t* out_w);

/* Re-pack torch-layout parameters into the kernels' layout.  weights[i]: device float32
 * [cout_i, cin_i, 3, 3]; biases[i]: device float32 [cout_i] (host arrays of device pointers, one per
 * convolution).  packed: device buffer of spr_vgg16_packed_bytes(). */
size_t spr_vgg16_packed_bytes(const spr_vgg16_plan* plan);
int spr_vgg16_pack_weights(spr_vgg16_plan* plan, const float* const* weights, const float* const* biases,
                           void* packed, spr_stream_t stream);

/* Forward pass of n images.  images: device uint8, [n, in_h, in_w] (in_channels = 1: the grey value is
 * repeated over the 3 input planes, network.py:67) or [n, in_h, in_w, 3] (in_channels = 3, RGB).
 * workspace: device buffer of spr_vgg16_workspace_bytes(); out: device float32 [n, C, h, w] (NCHW, the
 * layout Model.get_feature_maps returns per image, network.py:241-244). */
size_t spr_vgg16_workspace_bytes(const spr_vgg16_plan* plan, int64_t n, int32_t in_h, int32_t in_w);
int spr_vgg16_forward(spr_vgg16_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                      int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed,
                      void* workspace, float* out, spr_stream_t stream);

/* As spr_vgg16_forward, and convolution tap_convs[t] (ordinal among the plan's convolutions, not the first one) also
 * writes its activation - after bias / BatchNorm / ReLU, BEFORE any max-pool fused behind it - to tap_out[t] as float32
 * NCHW [n, cout, h, w] of that layer.  One pass of the extractor then feeds a multi-layer score (BASELINE config 5:
 * conv3_3 + conv4_3 + conv5_3 = convolutions 6, 9 and 12 of features[:30]; the reference runs one block per cluster,
 * run.py:20). */
int spr_vgg16_forward_taps(spr_vgg16_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                           int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed,
                           void* workspace, float* out, int32_t n_taps, const int32_t* tap_convs, float* const* tap_out,
                           spr_stream_t stream);

/* Per-layer trace of a plan, for tests (the record format and the contract are spr_resnet_trace_layout's and
 * spr_resnet_forward_trace's, below): spr_vgg16_forward_trace is spr_vgg16_forward_taps - the same kernels, the same `out`,
 * the same taps - that also copies, behind every stage and on the same stream, what that stage stored into `trace`.  One
 * record per convolution of spr_vgg16_conv_shape's list, in that order:
 *   record 0                 the first convolution's output (bias, ReLU): NHWC [n][h][w][64] in the plan's compute type
 *   record i, 0 < i < last   what stage i stored, behind bias / ReLU / the fused 2x2 max pool: NHWC [n][h_i][w_i][cout_i] in
 *                            the plan's compute type (float32 for a float32 plan)
 *   the last record          the float32 NCHW output [n][C][h][w], i.e. `out`
 * An SPR_COMPUTE_BF16X3 plan's records 0 .. last - 1 carry type code 3 and hold the stored words as they are: 4 bytes per
 * channel in the hi / lo layout of spr_vgg_plan_create_ex.
 * A float32 plan that is its first convolution alone has that one NCHW record.  Refused with SPR_ERR_UNSUPPORTED by both
 * entry points: a 16-bit plan that consists of its first convolution alone (it runs in float32, see spr_vgg_plan_create_ex,
 * and stores no 16-bit record).  SPR_ERR_SHAPE: the image vanishes under the pools. */
int spr_vgg16_trace_layout(const spr_vgg16_plan* plan, int64_t n, int32_t in_h, int32_t in_w, int64_t* records,
                           size_t* total_bytes);
int spr_vgg16_forward_trace(spr_vgg16_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                            int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed,
                            void* workspace, float* out, int32_t n_taps, const int32_t* tap_convs, float* const* tap_out,
                            void* trace, spr_stream_t stream);

/* ------------------------------------------------------------------ RGB route of CLAHE (network.py:199-204)
 * The reference equalises a colour image on its L channel: cv2.cvtColor(RGB2LAB) -> CLAHE(L) -> cv2.cvtColor(LAB2RGB).
 * 8-bit convention (L * 255/100, a + 128, b + 128; sRGB, D65); interleaved uint8 [n_pixels, 3] in and out.  `tables`:
 * device buffer of spr_color_tables_bytes() bytes filled by the caller (int32: 256 gamma, 3072 cube-root, 9 matrix,
 * 4096 inverse-gamma entries; shoeprint_image_retrieval_amd/color.py builds them).  Parity with OpenCV itself is
 * unpinned (no cv2 offline): the kernels are bit-identical to oracle/color_oracle.py. */
size_t spr_color_tables_bytes(void);
int spr_rgb_to_lab_u8(const uint8_t* rgb, uint8_t* lab, int64_t n_pixels, const void* tables, spr_stream_t stream);
int spr_lab_to_rgb_u8(const uint8_t* lab, uint8_t* rgb, int64_t n_pixels, const void* tables, spr_stream_t stream);

/* ------------------------------------------------------------------ ResNet50 extractor (build-defined)
 * BASELINE.json config 3 asks for "ResNet50 layer3 summed maps"; the reference has no ResNet branch (network.py:121-182)
 * and its truncation rule `list(model.features.children())[:block]` (network.py:185) has no `.features` to act on there.
 * Defined here as torchvision's resnet50 (v1.5: stride on the 3x3 convolution) cut after `block` of its top-level children
 * [conv1, bn1, relu, maxpool, layer1, layer2, layer3]: block = 5 / 6 / 7 -> [256|512|1024, H/4|H/8|H/16, W/4|W/8|W/16].
 * Same calling sequence as the VGG plan: conv shapes in module order (conv1; per bottleneck conv1, conv2, conv3 and, in a
 * layer's first block, the downsample convolution), weights [cout][cin][k][k] + bias with eval-mode BatchNorm folded in
 * by the caller, packed once; forward = pre-processing (network.py:60-71) + stem + max pool + bottlenecks on the fp32
 * matrix cores, float32 NCHW out.  role: 0 stem, 1/2/3 a bottleneck's convolutions, 4 downsample. */
typedef struct spr_resnet_plan spr_resnet_plan;
int spr_resnet_plan_create(int32_t block, spr_resnet_plan** plan_out);
/* With a compute type, as spr_vgg_plan_create_ex: SPR_F32 (the f32 matrix cores) or SPR_F16 / SPR_BF16 - every convolution,
 * the 7x7 stem included (its operand is the normalised image), on v_mfma_f32_16x16x32 with its (BatchNorm-folded) weights and
 * the activations between layers, the residual operand included, rounded to that type; f32 accumulation, bias, residual sum
 * and ReLU; the float32 NCHW output is unchanged (BASELINE config 3: "ResNet50 layer3 summed maps, bf16"). */
int spr_resnet_plan_create_ex(int32_t block, int32_t compute, spr_resnet_plan** plan_out);
int spr_resnet_plan_compute(const spr_resnet_plan* plan);
void spr_resnet_plan_destroy(spr_resnet_plan* plan);
int spr_resnet_num_convs(const spr_resnet_plan* plan);
int spr_resnet_conv_shape(const spr_resnet_plan* plan, int32_t i, int32_t* cin, int32_t* cout, int32_t* ksize,
                          int32_t* stride, int32_t* role);
int spr_resnet_output_shape(const spr_resnet_plan* plan, int32_t in_h, int32_t in_w, int32_t* channels, int32_t* out_h,
                            int32_t* out_w);
size_t spr_resnet_packed_bytes(const spr_resnet_plan* plan);
int spr_resnet_pack_weights(spr_resnet_plan* plan, const float* const* weights, const float* const* biases, void* packed,
                            spr_stream_t stream);
size_t spr_resnet_workspace_bytes(const spr_resnet_plan* plan, int64_t n, int32_t in_h, int32_t in_w);
int spr_resnet_forward(spr_resnet_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                       int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed, void* workspace,
                       float* out, spr_stream_t stream);
/* Per-layer trace of a plan of any compute type (a float32 plan stores float32 records), for tests: spr_*_forward_trace
 * is the plain forward (the same kernels, the same result in `out`) that also copies, behind every layer and on the same
 * stream, what that layer stored into the device buffer `trace`.  spr_*_trace_layout(plan, n, in_h, in_w, records, total_bytes) returns the number of
 * records and, where the pointers are not null, int64 records[6 * i ..] = byte offset into `trace`, h, w, channels, element
 * type (SPR_F16 | SPR_BF16 | SPR_F32), layout (0 NHWC: [n][h][w][channels], padded channels included; 1 NCHW: the float32
 * output of the last layer, real channels) and the size of `trace` in bytes.  ResNet records: the stem's output before the
 * max pool, the max pool's output, then one per convolution of spr_resnet_conv_shape's list, in that (conv index) order. */
int spr_resnet_trace_layout(const spr_resnet_plan* plan, int64_t n, int32_t in_h, int32_t in_w, int64_t* records,
                            size_t* total_bytes);
int spr_resnet_forward_trace(spr_resnet_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                             int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed, void* workspace,
                             float* out, void* trace, spr_stream_t stream);
/* Feature taps of the ResNet50, EfficientNet and DenseNet plans: spr_*_forward_taps is spr_*_forward (the same kernels, the
 * same `out`, the same workspace) that also hands out the activation at n_taps further slice ends: tap_features[t] is an end
 * into the backbone's children like the plan's block and strictly below it, tap_out[t] a device float32 [n, C_t, h_t, w_t]
 * buffer of the caller's whose shape spr_*_tap_shape reports.  One pass then feeds a multi-layer score, as
 * spr_vgg16_forward_taps does for the plain VGGs.
 * The contract, for every family: the tap at end t of a plan truncated at block >= t is bit for bit the `out` of a plan of the
 * same arch, compute type and parameters truncated at t.  In a 16-bit plan it is therefore the unrounded float32 value, and
 * what the tapped layer stores for the next one is its rounding to the plan's type.  The block-end convolution stores both
 * forms from the same accumulators (ResNet, EfficientNet); DenseNet's block tensors leave through the plan's closing kernel.
 * Accepted ends - ResNet50: 5, 6 (layer1, layer2) below the block; EfficientNet: every stage end 2 .. block - 1 (not the stem
 * alone); DenseNet_201: 5 .. block - 1.  Anything else, a tap named twice or a tap >= block: SPR_ERR_ARG with the accepted
 * values in the message, and nothing is launched. */
int spr_resnet_tap_shape(const spr_resnet_plan* plan, int32_t tap_feature, int32_t in_h, int32_t in_w, int32_t* channels,
                         int32_t* out_h, int32_t* out_w);
int spr_resnet_forward_taps(spr_resnet_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                            int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed, void* workspace,
                            float* out, int32_t n_taps, const int32_t* tap_features, float* const* tap_out, spr_stream_t stream);

/* ------------------------------------------------------------------ EfficientNetV2 feature extractor
 * network.py:163-175 (model choice), :185-186 (`list(model.features.children())[:block]`), :60-71 / :74-87 (transforms).
 * arch: 0 = EfficientNetV2_S, 1 = EfficientNetV2_M (the reference's run.toml default), 2 = EfficientNetV2_L, 3 .. 8 =
 * EfficientNet_B1, B2, B3, B4, B5, B7 (network.py:139-162); block in [1, stages + 2] = [1, len(model.features)]: the stem, block - 1
 * stages and, with the last value, the closing 1x1 convolution of torchvision's efficientnet / efficientnet_v2.
 * The plan flattens the graph into layers (spr_effnet_op_info: int32[16] = kind {0 convolution, 1 depthwise 3x3, 2 squeeze-
 * excitation}, cin, cout, cin_p, cout_p, ksize, stride, act {0 none, 2 SiLU}, res, sq, feature index, offsets in floats of
 * w, b, w2, b2 in the packed buffer, block_end).  The caller folds eval-mode BatchNorm (eps 1e-3) into the convolutions and writes
 * the packed buffer itself (device, spr_effnet_packed_bytes):
 *   convolution      w at [cout_p/64][K/16][64][16] with K = tap * cin_p + c (zero where padded), b [cout_p]
 *   depthwise        w [9][c_p], b [c_p]
 *   squeeze-excite   w = fc1 [sq][c_p], b = fc1 bias [sq], w2 = fc2 [c_p][sq], b2 = fc2 bias [c_p]
 * images / mean3 / inv_std3 / out as for spr_vgg16_forward (out: device float32 [n, C, h, w], real channels only). */
typedef struct spr_effnet_plan spr_effnet_plan;
int spr_effnet_plan_create(int32_t arch, int32_t block, spr_effnet_plan** plan_out);
/* With a compute type (as spr_vgg_plan_create_ex): SPR_F16 / SPR_BF16 run every convolution on v_mfma_f32_16x16x32 with the
 * activations between layers stored in that type (the stem reads the rounded normalised image; squeeze-excitation means,
 * factors and the depthwise weights stay f32).  The caller then packs, at the same offsets:
 *   stem             w as 16-bit [k / 8][64][8], k = tap * 3 + plane (zero for k >= 27 and for padded channels), b f32 [64]
 *   convolution      w as 16-bit [cout_p/64][K/64][64][64] with K = tap * cin_p + c, b f32 [cout_p]
 *   depthwise / squeeze-excitation   as in the f32 plans
 * A plan that is the stem alone (block 1) must be f32. */
int spr_effnet_plan_create_ex(int32_t arch, int32_t block, int32_t compute, spr_effnet_plan** plan_out);
int spr_effnet_plan_compute(const spr_effnet_plan* plan);
void spr_effnet_plan_destroy(spr_effnet_plan* plan);
int spr_effnet_num_ops(const spr_effnet_plan* plan);
int spr_effnet_op_info(const spr_effnet_plan* plan, int32_t i, int32_t* info16);
int spr_effnet_output_shape(const spr_effnet_plan* plan, int32_t in_h, int32_t in_w, int32_t* channels, int32_t* out_h,
                            int32_t* out_w);
size_t spr_effnet_packed_bytes(const spr_effnet_plan* plan);
size_t spr_effnet_workspace_bytes(const spr_effnet_plan* plan, int64_t n, int32_t in_h, int32_t in_w);
int spr_effnet_forward(spr_effnet_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                       int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed, void* workspace,
                       float* out, spr_stream_t stream);
/* Per-layer trace (see spr_resnet_forward_trace), one record per layer of the plan in order: the stem and every convolution /
 * depthwise convolution as stored (NHWC in the plan's compute type, cout_p channels), a squeeze-excitation's float32 factors
 * [n][cin_p] (h = w = 1), the last layer's float32 NCHW output. */
int spr_effnet_trace_layout(const spr_effnet_plan* plan, int64_t n, int32_t in_h, int32_t in_w, int64_t* records,
                            size_t* total_bytes);
int spr_effnet_forward_trace(spr_effnet_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                             int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed, void* workspace,
                             float* out, void* trace, spr_stream_t stream);
/* Feature taps (see spr_resnet_forward_taps): every stage end 2 .. block - 1 of model.features. */
int spr_effnet_tap_shape(const spr_effnet_plan* plan, int32_t tap_feature, int32_t in_h, int32_t in_w, int32_t* channels,
                         int32_t* out_h, int32_t* out_w);
int spr_effnet_forward_taps(spr_effnet_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                            int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed, void* workspace,
                            float* out, int32_t n_taps, const int32_t* tap_features, float* const* tap_out, spr_stream_t stream);

/* ------------------------------------------------------------------ DenseNet_201 feature extractor
 * network.py:176-179, :185-186: torchvision's densenet201 `features` = [conv0, norm0, relu0, pool0, denseblock1, transition1,
 * denseblock2, transition2, denseblock3, transition3, denseblock4, norm5], truncated to features[:block], block in [1, 12].
 * spr_densenet_op_info: int32[12] = kind {0 stem, 1 dense 1x1, 2 dense 3x3, 3 transition, 4 closing BatchNorm}, cin, cout,
 * c_off, ctot, flags {stem: 1 BatchNorm folded, 2 ReLU, 4 max pool}, feature index, offsets in floats of w, b, s, t in the
 * packed buffer, 0.  The caller writes the packed buffer (device, spr_densenet_packed_bytes):
 *   stem        w [tap * 3 + c][64] (norm0 folded when flag 1), b [64]
 *   dense 1x1   s, t [cin] = the BatchNorm in front of it as x * s + t (ReLU follows); w GEMM-packed [128/64][cin/16][64][16]
 *               with the second BatchNorm folded, b [128]
 *   dense 3x3   w GEMM-packed [1][9 * 128 / 16][64][16] (output channels 32 .. 63 zero), b [64] zeros
 *   transition  s, t [cin]; w GEMM-packed [cout/64][cin/16][64][16], b [cout] zeros
 *   closing     s, t [C]
 * images / mean3 / inv_std3 / out as for spr_vgg16_forward. */
typedef struct spr_densenet_plan spr_densenet_plan;
int spr_densenet_plan_create(int32_t block, spr_densenet_plan** plan_out);
/* With a compute type (as spr_effnet_plan_create_ex): SPR_F32 is spr_densenet_plan_create's plan; SPR_F16 / SPR_BF16, for
 * block in [5, 12] (a plan that ends inside the stem must be f32: SPR_ERR_UNSUPPORTED), run every convolution on
 * v_mfma_f32_16x16x32 with every tensor between layers stored in that type; the pre-activation scales / shifts, the biases,
 * the accumulation, the average pool's sum and the closing BatchNorm stay f32 (the list of rounding points: densenet.hip).
 * The caller then packs, at the offsets spr_densenet_op_info reports (floats) and with the sizes of that plan:
 *   stem        w as 16-bit [k / 8][64][8], k = tap * 3 + plane, zero for k in [147, 160) (norm0 folded), b f32 [64]
 *   dense 1x1   s, t f32 [cin]; w as 16-bit [2][ceil(cin / 64)][64][64] (second BatchNorm folded, zero behind cin), b f32 [128]
 *   dense 3x3   w as 16-bit [1][9 * 2][32][64], K index = tap * 128 + c; b f32 [32] zeros
 *   transition  s, t f32 [cin]; w as 16-bit [cout / 64][cin / 64][64][64], b f32 [cout] zeros
 *   closing     s, t f32 [C] */
int spr_densenet_plan_create_ex(int32_t block, int32_t compute, spr_densenet_plan** plan_out);
int spr_densenet_plan_compute(const spr_densenet_plan* plan);
void spr_densenet_plan_destroy(spr_densenet_plan* plan);
int spr_densenet_num_ops(const spr_densenet_plan* plan);
int spr_densenet_op_info(const spr_densenet_plan* plan, int32_t i, int32_t* info12);
int spr_densenet_output_shape(const spr_densenet_plan* plan, int32_t in_h, int32_t in_w, int32_t* channels, int32_t* out_h,
                              int32_t* out_w);
size_t spr_densenet_packed_bytes(const spr_densenet_plan* plan);
size_t spr_densenet_workspace_bytes(const spr_densenet_plan* plan, int64_t n, int32_t in_h, int32_t in_w);
int spr_densenet_forward(spr_densenet_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                         int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed, void* workspace,
                         float* out, spr_stream_t stream);
/* Per-layer trace (see spr_resnet_forward_trace).  Records, all NHWC in the plan's compute type but the last: the stem's output;
 * block 1's tensor behind the max pool (its first 64 channels are written, the rest is whatever the workspace held); per
 * dense layer its 128-channel intermediate; per dense block its complete tensor behind the last layer (slices are never
 * overwritten: it holds every 3x3 result and every later layer's input); per transition its convolution's result and the
 * next tensor behind the average pool (its first cout channels are written); the float32 NCHW output. */
int spr_densenet_trace_layout(const spr_densenet_plan* plan, int64_t n, int32_t in_h, int32_t in_w, int64_t* records,
                              size_t* total_bytes);
int spr_densenet_forward_trace(spr_densenet_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                               int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed, void* workspace,
                               float* out, void* trace, spr_stream_t stream);
/* Feature taps (see spr_resnet_forward_taps): the ends 5 .. block - 1 of model.features (behind a dense block or a
 * transition).  The tap is the plan's closing layout kernel launched on the live block tensor (behind a transition: on what
 * the transition stored), so in a 16-bit plan it holds the stored values, as the truncated plan's output does. */
int spr_densenet_tap_shape(const spr_densenet_plan* plan, int32_t tap_feature, int32_t in_h, int32_t in_w, int32_t* channels,
                           int32_t* out_h, int32_t* out_w);
int spr_densenet_forward_taps(spr_densenet_plan* plan, const uint8_t* images, int64_t n, int32_t in_h, int32_t in_w,
                              int32_t in_channels, const float* mean3, const float* inv_std3, const void* packed, void* workspace,
                              float* out, int32_t n_taps, const int32_t* tap_features, float* const* tap_out,
                              spr_stream_t stream);

/* ------------------------------------------------------------------ synthetic data
 * Bench/test support: the device twin of shoeprint_image_retrieval_amd/synth.py (bit-identical
 * float32 values).  out: device float32 [n, C, h, w]. */
int spr_synth_gallery(float* out, int64_t first_item, int64_t n, int32_t channels, int32_t h,
                      int32_t w, uint64_t seed, spr_stream_t stream);
/* match: device int32 [n] = gallery index each query is derived from. */
int spr_synth_queries(float* out, int64_t first_query, int64_t n, const int32_t* match,
                      int32_t channels, int32_t h, int32_t w, uint64_t seed, int32_t max_shift,
                      int32_t signal, int32_t noise, spr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SHOEPRINT_MI355X_H */
