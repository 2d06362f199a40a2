/* pointslot_hip.h — C-ABI of libpointslot_hip.so: the MI355X (gfx950) implementation of the SLOT
 * front-end / back-end hot path of pkzhou/PointSLOT.
 *
 * The reference has no FFI layer: callers use the C++ classes ORB_SLAM2::ORBextractor, ORBmatcher
 * and Optimizer directly.  This header is the boundary a maintainer would
 * bind from those classes (the shim classes are in pointslot_amd/host/, the recipe in
 * INTEGRATION.md).  Every entry point cites the reference function it replaces.
 *
 * Conventions: plain C, POD structs, caller-owned buffers, no exceptions.  Every function returns
 * PS_OK (0) or a negative ps_status.  Handles are not re-entrant (like an ORBextractor instance,
 * which owns mvImagePyramid); distinct handles may be used from distinct threads concurrently.
 * Pointers named d_* are device (HBM) pointers, everything else is host memory.
 */
#ifndef POINTSLOT_HIP_H
#define POINTSLOT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum ps_status {
  PS_OK = 0,
  PS_ERR_INVALID = -1,   /* bad argument (null pointer, non-positive size, unsupported shape) */
  PS_ERR_HIP = -2,       /* a HIP runtime call failed; ps_last_error() has the text          */
  PS_ERR_CAPACITY = -3,  /* caller buffer or plan capacity too small                          */
  PS_ERR_NO_DEVICE = -4  /* no gfx950 device visible                                          */
} ps_status;

/* Binary-compatible with cv::KeyPoint (OpenCV 3.x): pt.x, pt.y, size, angle, response, octave,
 * class_id — 28 bytes.  Filled exactly as ORBextractor::operator() fills it
 * (/root/reference/src/ORBextractor.cc:837-852,1095-1101). */
typedef struct ps_keypoint {
  float x, y;
  float size;
  float angle;
  float response;
  int32_t octave;
  int32_t class_id;
} ps_keypoint;

const char* ps_last_error(void);
int ps_device_count(int* count);
const char* ps_version(void);
/* Test / diagnostic: fills the LDS of every CU of `device` with the 32-bit `pattern` (e.g. 0xFFFFFFFF: NaN when read as floating
 * point) and leaves it there.  LDS is not cleared between kernels, so a kernel that reads LDS it never wrote - or multiplies such
 * a slot by zero - then misbehaves deterministically instead of once in a while; the GPU tests call this before the kernels. */
int ps_debug_poison_lds(int device, uint32_t pattern);
/* Diagnostic: measured FP64 matrix-core rate of `device` in TFLOP/s (a loop of independent v_mfma_f64_16x16x4_f64 on every CU).
 * The local hardware guide has no FP64 MFMA peak; this is the denominator of the object-BA roofline. */
int ps_debug_mfma_f64_peak(int device, double* tflops);
/* Diagnostic: `repeats` launches of a streaming kernel that touches exactly `bytes` of a fresh buffer once per launch - mode 0 reads
 * 16 B per lane, 1 reads 4 B per lane, 2 writes 4 B per lane, 3 writes 16 B per lane (kernel names traffic_read / traffic_write).
 * Run under `rocprofv3 --pmc FETCH_SIZE` / `WRITE_SIZE` it calibrates those counters for the access widths the kernels of this
 * library use (the hardware guide only calibrates 16-byte reads); tools/pmc_traffic.sh applies the factors. */
int ps_debug_traffic_kernel(int device, int mode, size_t bytes, int repeats);
/* Page-locked host memory for image and result buffers: copies from/to it are asynchronous and run at full PCIe rate
 * (ps_orb_extract_batch reads the caller's image buffers directly).  NULL on failure (ps_last_error has the text). */
void* ps_pinned_alloc(size_t bytes);
void ps_pinned_free(void* p);

/* ------------------------------------------------------------------------------------------------
 * ORB extractor — replaces ORB_SLAM2::ORBextractor (/root/reference/include/ORBextractor.h:51-85,
 * src/ORBextractor.cc:410-470 ctor, :1043-1105 operator()).
 * ---------------------------------------------------------------------------------------------- */
typedef struct ps_orb ps_orb;

typedef struct ps_orb_config {
  int32_t nfeatures;      /* ORBextractor.nFeatures   (yaml: 1000; BASELINE config 2: 2000) */
  float scale_factor;     /* ORBextractor.scaleFactor (1.2)                                  */
  int32_t nlevels;        /* ORBextractor.nLevels     (8; 1..8 supported)                    */
  int32_t ini_th_fast;    /* ORBextractor.iniThFAST   (20)                                   */
  int32_t min_th_fast;    /* ORBextractor.minThFAST   (5)                                    */
  int32_t max_batch;      /* images processed per ps_orb_extract_batch_device call (>= 1)    */
  int32_t device;         /* HIP device ordinal                                              */
} ps_orb_config;

int ps_orb_create(const ps_orb_config* cfg, ps_orb** out);
void ps_orb_destroy(ps_orb* h);

/* Getters of ORBextractor.h:61-83.  Each array has nlevels entries; any pointer may be NULL. */
int ps_orb_get_tables(const ps_orb* h, float* scale_factors, float* inv_scale_factors,
                      float* level_sigma2, float* inv_level_sigma2, int32_t* features_per_level);

/* Level geometry for an image of w x h: level sizes (ORBextractor.cc:1111-1112).  The padded plane
 * of a level is (w_l + 38) x (h_l + 38) (EDGE_THRESHOLD = 19 on every side, :1113). */
int ps_orb_level_size(const ps_orb* h, int w, int hgt, int level, int32_t* w_l, int32_t* h_l);

/* ORBextractor::operator()(image, mask (ignored), keypoints, descriptors) for ONE host image.
 *   img/stride : CV_8UC1 image, `stride` bytes per row.  w <= 0 || hgt <= 0 || !img => *n = 0, PS_OK
 *                (the reference returns silently on an empty image, ORBextractor.cc:1046-1047).
 *   kps, desc  : caller buffers with room for `cap` keypoints / cap x 32 descriptor bytes.  The
 *                extractor may return up to nfeatures + 3 * nlevels keypoints (the quadtree stops
 *                at >= quota leaves per level, ORBextractor.cc:669-737).
 *   pyramid_out: NULL, or nlevels pointers; plane l receives the padded level image, tightly packed
 *                (w_l + 38) bytes per row — the contents of mvImagePyramid[l]'s parent buffer
 *                (ORBextractor.cc:1113-1128) that Frame::ComputeStereoMatches reads. */
int ps_orb_extract(ps_orb* h, const uint8_t* img, int w, int hgt, int stride, ps_keypoint* kps,
                   uint8_t* desc, int cap, int* n, uint8_t* const* pyramid_out);

/* The object features of a frame — Frame::ExtractObjORB -> OpencvORBDetector (/root/reference/src/Frame.cc:2623-2665):
 * cv::ORB::create(1000, 1.2, 8, 19)->detectAndCompute(im, ObjMask, kp, descriptor).  SURVEY.md 8f-2: OpenCV's own ORB (Harris
 * ranking, its own pyramid) is a different extractor; this entry point is the DECLARED STAND-IN - this library's pipeline on a
 * handle created with (1000, 1.2, 8, 20, 5), keypoints whose level-0 pixel lies outside `mask` (zero bytes) dropped before the
 * quadtree - so object keypoint sets differ from a true PointSLOT run.  mask == NULL: no mask. */
int ps_orb_extract_masked(ps_orb* h, const uint8_t* img, const uint8_t* mask, int w, int hgt, int stride, int mask_stride,
                          ps_keypoint* kps, uint8_t* desc, int cap, int* n);

/* ... and the detector itself: OpenCV 3.4.3's ORB_Impl::detectAndCompute (features2d/src/orb.cpp; firstLevel 0, WTA_K 2,
 * HARRIS_SCORE, patchSize 31) restated for the GPU - INTER_LINEAR_EXACT pyramid and mask pyramid (threshold 254 above level 0),
 * whole-image FAST-9/16 with non-maximum suppression, runByPixelsMask, runByImageBorder(edge_threshold), retainBest(2 N) by
 * FAST score, Harris responses (7 x 7, k = 0.04), retainBest(N), intensity-centroid angles, 7 x 7 sigma-2 blur, 256-bit rBRIEF.
 * Keypoints come out level by level in the order KeyPointsFilter::retainBest leaves them (std::nth_element / std::partition,
 * executed on the host with the same library calls).  UNVERIFIABLE against OpenCV in the build image, like every OpenCV stage of
 * the path; the CPU restatement it is tested against follows the same published source.
 * Frame.cc:2625: cv::ORB::create(1000, 1.2, 8, 19) == ps_cvorb_create(1000, 1.2f, 8, 19, 20, device, &h). */
typedef struct ps_cvorb ps_cvorb;
int ps_cvorb_create(int nfeatures, float scale_factor, int nlevels, int edge_threshold, int fast_threshold, int device, ps_cvorb** out);
void ps_cvorb_destroy(ps_cvorb* h);
/* detectAndCompute(image, mask, keypoints, descriptors); mask == NULL: no mask (non-zero mask bytes keep a keypoint). */
int ps_cvorb_detect_and_compute(ps_cvorb* h, const uint8_t* img, const uint8_t* mask, int w, int hgt, int stride, int mask_stride,
                                ps_keypoint* kps, uint8_t* desc, int cap, int* n);
/* Test access to intermediates of the last call.  what: 0 level image (tight w x h), 1 blurred level, 2 level mask, 3 the FAST
 * keypoints after the mask / border filters in raster order as float rows (x, y, score, Harris response), count in *n,
 * 4 the level size as int32[2]. */
int ps_cvorb_debug_read(ps_cvorb* h, int level, int what, void* out, size_t out_bytes, int* n);

/* Batched, device-resident form of ps_cvorb_detect_and_compute - Frame::ExtractObjORB for many frames at once: `nimg` images of one
 * size in HBM (image i at d_imgs + i * image_pitch) with their object masks (d_masks + i * mask_pitch, non-zero = keep), all
 * work queued on `stream` (a hipStream_t; NULL = the handle's stream) with nothing returning to the host: the two retainBest steps
 * run on the device with libstdc++'s own selection algorithms restated (csrc/retain_best.h), so the keypoints of an image are those
 * of the single-image call, order included.  Work is restricted to the parts of the pyramid a keypoint under the mask can touch.
 * Limits (reported as PS_ERR_CAPACITY by ps_cvorb_batch_fetch, never truncated silently): 2048 FAST keypoints under the mask per
 * level, 2048 keypoints per image.  Outputs stay in HBM: keypoints [nimg][capacity], descriptors [nimg][capacity][32], counts. */
int ps_cvorb_detect_batch_device(ps_cvorb* h, const uint8_t* d_imgs, const uint8_t* d_masks, int nimg, int w, int hgt, int stride,
                                 size_t image_pitch, int mask_stride, size_t mask_pitch, void* stream);
int ps_cvorb_batch_device_outputs(const ps_cvorb* h, const ps_keypoint** d_kps, const uint8_t** d_desc, const int32_t** d_counts,
                                  const int32_t** d_overflow, int32_t* capacity);
int ps_cvorb_batch_fetch(ps_cvorb* h, int image, ps_keypoint* kps, uint8_t* desc, int cap, int* n);

/* Batched, device-resident form of the same call: `nimg` images of identical size already in HBM
 * (image i at d_imgs + i * image_pitch, rows `stride` bytes apart).  Results stay in HBM inside the
 * handle; the call is asynchronous on `stream` (a hipStream_t, NULL = the handle's own stream). */
int ps_orb_extract_batch_device(ps_orb* h, const uint8_t* d_imgs, int nimg, int w, int hgt, int stride,
                                size_t image_pitch, void* stream);
/* Device views of the last batch: keypoints [nimg][kp_capacity], descriptors
 * [nimg][kp_capacity][32], counts [nimg]. */
int ps_orb_batch_device_outputs(const ps_orb* h, const ps_keypoint** d_kps, const uint8_t** d_desc,
                                const int32_t** d_counts, int32_t* kp_capacity);
/* Blocks until the batch is complete and copies image i's results to the host. */
int ps_orb_batch_fetch(ps_orb* h, int image, ps_keypoint* kps, uint8_t* desc, int cap, int* n);
/* Waits for all work queued on the handle. */
int ps_orb_sync(ps_orb* h);

/* The same batched extraction for images in HOST memory (nimg pointers, identical size, rows `stride` bytes apart): one
 * upload per image on the handle's stream, then the batch pipeline.  Asynchronous when the buffers come from
 * ps_pinned_alloc; results are read with ps_orb_batch_fetch / ps_orb_stereo_fetch_frames.  This is Frame::Frame's
 * ExtractORB(0, imLeft) + ExtractORB(1, imRight) (src/Frame.cc:709-712) for many frames at once: image 2k = left,
 * 2k+1 = right of frame k when ps_orb_stereo_match_batch follows. */
int ps_orb_extract_batch(ps_orb* h, const uint8_t* const* imgs, int nimg, int w, int hgt, int stride);

/* Frame::ComputeStereoMatches (/root/reference/src/Frame.cc:2142-2316) on extraction results that
 * are still in HBM: both padded pyramids (mvImagePyramid of the left and the right extractor), keypoints and descriptors.
 * mb = Frame::mb (baseline in metres), mbf = Frame::mbf.  Outputs are indexed like the LEFT image's keypoints:
 * u_right = mvuRight, depth = mvDepth, -1 where the keypoint has no stereo match.
 *   ps_orb_stereo_match_batch : the last batch of `h` holds left/right interleaved (image 2k = left, 2k+1 = right)
 *   ps_orb_stereo_match_pair  : the reference's layout — two extractor objects, one image each (Frame.cc:709-722) */
int ps_orb_stereo_match_batch(ps_orb* h, int npairs, float mb, float mbf);
int ps_orb_stereo_device_outputs(const ps_orb* h, const float** d_uright, const float** d_depth, const int32_t** d_kept);
int ps_orb_stereo_fetch(ps_orb* h, int pair, float* u_right, float* depth, int cap, int* n_left, int* kept);
int ps_orb_stereo_match_pair(ps_orb* left, ps_orb* right, float mb, float mbf, float* u_right, float* depth, int cap, int* n_left);
/* Everything a stereo Frame keeps from its two extractors and ComputeStereoMatches (mvKeys, mDescriptors, mvuRight,
 * mvDepth; src/Frame.cc:709-722), for the first `npairs` pairs of the last ps_orb_stereo_match_batch, in one
 * synchronisation and one pipelined transfer.  In: kps/desc/u_right/depth buffers with room for `cap` keypoints.
 * Out: n (left keypoints), n_right, kept (matches that survive the median cut). */
typedef struct ps_stereo_frame {
  ps_keypoint* kps; uint8_t* desc; float* u_right; float* depth;
  int32_t cap;
  int32_t n, n_right, kept;
} ps_stereo_frame;
int ps_orb_stereo_fetch_frames(ps_orb* h, ps_stereo_frame* frames, int npairs);
/* Frame::ComputeObjStereoMatches (src/Frame.cc:2318-2503): the same matcher on caller-provided key sets (the frame's object
 * features, mvTempObjKeys / mvTempObjKeysRight + descriptors, <= 4096 each) against the two extractors' device-resident
 * pyramids.  u_right / depth: n_left floats (-1 where unmatched); *kept (nullable) = matches that survive the median cut.
 * Keypoints must lie where the reference's 11x11 window + slide stays inside the level image (cv::ORB's edge threshold). */
int ps_orb_stereo_match_keys(ps_orb* left, ps_orb* right, const ps_keypoint* kps_l, const uint8_t* desc_l, int n_left,
                             const ps_keypoint* kps_r, const uint8_t* desc_r, int n_right, float mb, float mbf,
                             float* u_right, float* depth, int* kept);

/* Test/diagnostic access to intermediates of the last call (blocking).  `what`:
 *   0 padded plane (tight, (w_l+38) x (h_l+38) bytes)      1 blurred plane (tight, w_l x h_l)
 *   2 FAST candidates in reference emission order, int32 triples (x, y, score) relative to
 *     minBorder (ORBextractor.cc:822-824); returns the count in *n
 *   3 selected keypoints of the level, int32 triples (x, y, score) in level coordinates, in
 *     DistributeOctTree's output order; count in *n */
int ps_orb_debug_read(ps_orb* h, int image, int level, int what, void* out, size_t out_bytes, int* n);

/* Per-stage GPU time of ps_orb_extract_batch_device, measured with HIP events recorded on the stream
 * the kernels run on.  After ps_orb_enable_stage_timing(h, 1) every batch records one event set (a
 * ring of 64); ps_orb_stage_times synchronises and returns the mean over the recorded batches.
 * names/ms arrays of length `cap`; *n receives the stage count. */
int ps_orb_stage_times(ps_orb* h, const char** names, float* ms, int cap, int* n);
int ps_orb_enable_stage_timing(ps_orb* h, int enable);

/* ------------------------------------------------------------------------------------------------
 * Descriptor matching — replaces the hot members of ORB_SLAM2::ORBmatcher
 * (/root/reference/include/ORBmatcher.h:47-118, src/ORBmatcher.cc).
 * ---------------------------------------------------------------------------------------------- */
typedef struct ps_matcher ps_matcher;
int ps_matcher_create(int device, ps_matcher** out);
void ps_matcher_destroy(ps_matcher* m);
/* GPU time of the kernels of the last ps_match_bruteforce / ps_search_by_projection call (HIP events on the handle's stream). */
int ps_matcher_last_kernel_ms(const ps_matcher* m, float* ms);

/* Bulk form of ORBmatcher::DescriptorDistance (ORBmatcher.cc:2704-2720): out[i * nt + j] = Hamming
 * distance between 32-byte descriptors q[i] and t[j] (0..256). */
int ps_hamming_matrix(ps_matcher* m, const uint8_t* q, int nq, const uint8_t* t, int nt, uint16_t* out);

/* ORBmatcher::SearchByBruceMatching(LastFrame, CurrentFrame, nLastOrder, nCurrenOrder, matches)
 * (ORBmatcher.cc:2043-2155) for a batch of independent (object) problems.
 *   q_*   : the last frame's object features of one object: 32-byte descriptors
 *           (mvObjPointsDescriptors), angles of mvObjKeysUn, and q_valid[i] = 1 iff
 *           mvpMapObjectPoints[i] is non-null, not bad, and mvbObjKeysOutlier[i] is false (:2062-2063)
 *   t_*   : the current frame's features of the same object: descriptors, angles of mvObjKeys
 *   query_of_train[j] : out, index i of the query whose MapObjectPoint* the reference stores in
 *           vpMapObjectPointMatches[j], or -1 (NULL)
 *   nmatches : out, the function's return value
 * nn_ratio / check_orientation are the ORBmatcher constructor arguments (mfNNratio, mbCheckOrientation);
 * TH_LOW = 50 and HISTO_LENGTH = 30 are fixed as in ORBmatcher.cc:58-62. nt <= 4096. */
/* MapPoint / MapObjectPoint::ComputeDistinctiveDescriptors (src/MapObjectPoint.cc:379-436, src/MapPoint.cc:366; SURVEY.md
 * 8f-4) for a batch of points: point p owns the descriptor rows [off[p], off[p+1]) (its observations, <= 128);
 * best[p] = row index (relative to off[p]) of the descriptor with the least median distance to the others, -1 if none. */
int ps_distinctive_descriptors(ps_matcher* m, const uint8_t* desc, const int32_t* off, int npoints, int32_t* best);

typedef struct ps_bf_problem {
  const uint8_t* q_desc; const float* q_angle; const uint8_t* q_valid; int32_t nq;
  const uint8_t* t_desc; const float* t_angle; int32_t nt;
  int32_t* query_of_train;
  int32_t nmatches;
} ps_bf_problem;
int ps_match_bruteforce(ps_matcher* m, ps_bf_problem* probs, int nprob, float nn_ratio, int check_orientation);

/* The three ORBmatcher::SearchByProjection overloads as one windowed-matching call, batched:
 *   frame_mode = 1 : SearchByProjection(CurrentFrame, LastFrame, th, bMono)              (ORBmatcher.cc:1613-1756)
 *   frame_mode = 0 : SearchByProjection(F, vpMapPoints, th)                              (:68-155)  and
 *                    SearchByProjection(F, nOrder, vpMapObjectPoints, th) (use_bbox = 1) (:157-248)
 * `train` is the frame being matched INTO (CurrentFrame / F, or one object's feature set of it):
 *   x, y, octave, angle : mvKeysUn (mvObjKeysUn[nOrder]);  u_right : mvuRight;  desc : mDescriptors rows
 *   occupied[j] : 1 iff mvpMapPoints[j] is non-null AND has Observations() > 0 (the reference's skip test)
 *   in_bbox[j]  : Frame::isInBBox(nOrder, x, y) (object variant only)
 *   cell_off / cell_idx : mGrid as CSR, cell = ix * 48 + iy (FRAME_GRID_ROWS), indices in insertion order
 *   min_x, min_y, grid_w_inv, grid_h_inv : mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv
 * Queries are the points being projected, in the reference's loop order:
 *   q_valid    : frame mode: mvpMapPoints[i] && !mvbOutlier[i] of the LAST frame; else mbTrackInView && !isBad()
 *   q_desc     : pMP->GetDescriptor();   q_observed[i] : pMP->Observations() > 0
 *   frame mode : q_xw = GetWorldPos, q_octave = LastFrame.mvKeys[i].octave, q_angle = LastFrame.mvKeysUn[i].angle,
 *                tcw / tlw = CurrentFrame.mTcw / LastFrame.mTcw, fx..mb, bounds = mnMinX,mnMaxX,mnMinY,mnMaxY,
 *                scale_factors = mvScaleFactors, th, mono
 *   otherwise  : q_u, q_v, q_ur = mTrackProjX, mTrackProjY, mTrackProjXR; q_radius = window half-size
 *                (r * scaleFactor[level], or 5 for objects); q_radius_er = r * scaleFactor[level] (uR gate);
 *                q_min_level / q_max_level = level-1 / level (level+1 for objects)
 * th_dist = TH_HIGH (100) or TH_HIGH_FORDYNAMIC (130); ratio_test/nn_ratio = the same-level mfNNratio test;
 * check_orientation = mbCheckOrientation (frame mode).
 *   match_of_train[j] : out, index of the query assigned to slot j; -1 where the call leaves the slot alone (the caller keeps
 *                       its pointer); -2 where the call assigned the slot and the rotation check then reset it to NULL
 *                       (ORBmatcher.cc:1742-1750: the caller writes NULL)
 *   nmatches          : out, the return value
 * A search window may hold any number of candidates in the reference.  Here a window of more than 256 makes its problem run a
 * second time with a wider candidate store (1024 per window, frames of up to 8191 features); only a problem that exceeds that as
 * well fails - nmatches = -1, match_of_train untouched - and the call returns PS_ERR_CAPACITY after serving all other problems. */
typedef struct ps_proj_train {
  int32_t n;
  const float* x; const float* y; const int32_t* octave; const float* angle; const float* u_right; const uint8_t* desc;
  const uint8_t* occupied; const uint8_t* in_bbox;
  const int32_t* cell_off; const int32_t* cell_idx;
  float min_x, min_y, grid_w_inv, grid_h_inv;
} ps_proj_train;
typedef struct ps_proj_problem {
  ps_proj_train train;
  int32_t nq;
  const uint8_t* q_valid; const uint8_t* q_desc; const uint8_t* q_observed; const float* q_angle;
  const float* q_u; const float* q_v; const float* q_ur; const float* q_radius; const float* q_radius_er;
  const int32_t* q_min_level; const int32_t* q_max_level;
  const float* q_xw; const int32_t* q_octave;
  int32_t frame_mode, mono;
  float tcw[16], tlw[16];
  float fx, fy, cx, cy, mbf, mb;
  float bounds[4];
  float scale_factors[8];
  float th;
  int32_t th_dist, ratio_test; float nn_ratio; int32_t check_orientation, use_bbox;
  int32_t* match_of_train;
  int32_t nmatches;
} ps_proj_problem;
int ps_search_by_projection(ps_matcher* m, ps_proj_problem* probs, int nprob);

/* The search half of ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:982-1136) and
 * Fuse(ObjectKeyFrame*, const vector<MapObjectPoint*>&, th) (:1138-1260), SURVEY.md 8f-4: for every candidate point the
 * projection into the keyframe, the depth / image-or-box / scale-invariance / viewing-angle gates, PredictScale,
 * KeyFrame::GetFeaturesInArea(u, v, th * scale[level]) and the chi-square-gated (7.8 stereo / 5.99 mono) best Hamming match.
 * best_idx[i] = keyframe feature to fuse with (bestDist <= TH_LOW), -1 otherwise; best_dist[i] = bestDist (256 if none).
 * What the reference does next (Replace / AddObservation, :1113-1131 / :1239-1255) is map surgery and stays with the caller,
 * in candidate order.  train: the keyframe's mvKeysUn / mvObjKeysUn (x, y, octave), mvuRight, descriptors and feature grid
 * (angle / occupied / in_bbox unused).  q_valid[i] = pMP && !pMP->isBad() && !pMP->IsInKeyFrame(pKF); q_pos = GetWorldPos()
 * or GetInObjFramePosition(); q_min_dist / q_max_dist = mfMinDistance / mfMaxDistance (the 0.8 / 1.2 factors are applied
 * inside).  bounds = {minX, maxX, minY, maxY}: IsInImage's mnMin/MaxX/Y or IsInBBox's detection box (doubles, as there). */
typedef struct ps_fuse_problem {
  ps_proj_train train;
  int32_t nq;
  const uint8_t* q_valid;
  const float* q_pos;        /* [nq][3] */
  const float* q_normal;     /* [nq][3] GetNormal() */
  const float* q_min_dist;
  const float* q_max_dist;
  const uint8_t* q_desc;     /* [nq][32] GetDescriptor() */
  float rcw[9], tcw[3], ow[3];   /* GetRotation() row-major, GetTranslation(), GetCameraCenter() */
  float fx, fy, cx, cy, bf;
  double bounds[4];
  float scale_factors[8], inv_level_sigma2[8];
  float log_scale_factor;    /* mfLogScaleFactor */
  int32_t n_levels;          /* mnScaleLevels */
  float th;
  int32_t* best_idx;         /* out [nq] */
  int32_t* best_dist;        /* out [nq] */
} ps_fuse_problem;
int ps_fuse_search(ps_matcher* m, ps_fuse_problem* problems, int nproblems);

/* ------------------------------------------------------------------------------------------------
 * Frame handle — "this frame is already on the device".  A stereo Frame's search-relevant state, kept in HBM between the calls
 * that search into it: what Frame::Frame leaves in mvKeysUn, mvuRight, mDescriptors and mGrid
 * (/root/reference/src/Frame.cc:709-722, AssignFeaturesToGrid :1636-1656, PosInGrid :2027-2037).  The tracking thread searches
 * into the same frame two or three times (src/Tracking.cc:3047, :3305-3355, :2571); with a handle the train side of those calls -
 * x / y / octave / angle / u_right, the descriptors and the 64 x 48 grid as CSR, laid out exactly as ps_proj_train documents
 * them - is published once and neither rebuilt nor uploaded per call.
 *
 * Lifetimes and ordering.  The caller owns a handle from ps_frame_create to ps_frame_destroy; nothing is allocated in between.
 * A publish replaces the content and records a "ready" event; a search that reads the handle makes its stream wait for that
 * event and records a "last use" event behind its kernels; the next publish into the handle, and ps_frame_destroy, wait for the
 * last uses.  Any number of matcher handles on any number of threads may read one frame handle at the same time.  Publishing
 * is exclusive: do not publish into a handle while another thread starts a search on it, and expect every search queued after
 * a publish to see the new frame.  A tracker keeps two handles - current frame and last frame - and alternates between them.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ps_frame ps_frame;
/* capacity: the most keypoints a publish may carry, 1..32767.  One device slab, one pinned staging block, a stream and events. */
int ps_frame_create(int device, int capacity, ps_frame** out);
void ps_frame_destroy(ps_frame* f);
/* From host arrays: kps = mvKeysUn (cv::KeyPoint layout), u_right = mvuRight (NULL: monocular, all -1), desc = mDescriptors rows,
 * min_x .. grid_h_inv = mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv.  One staged asynchronous upload and one
 * kernel; returns as soon as both are queued.  n > capacity: PS_ERR_CAPACITY. */
int ps_frame_publish_host(ps_frame* f, const ps_keypoint* kps, const float* u_right, const uint8_t* desc, int n,
                          float min_x, float min_y, float grid_w_inv, float grid_h_inv);
/* From an extractor handle's last results, which are still in HBM (ps_orb_batch_device_outputs / ps_orb_stereo_device_outputs):
 * no host round trip, one launch for all frames (per 16).  image[k] = the left image's index in the batch, pair[k] = its index
 * in the stereo outputs or -1 for none (all u_right -1), n[k] = the keypoint count the caller has already fetched.  The batched
 * handle has image 2k / pair k; the reference's two-extractor layout has image 0 / pair 0 on the LEFT handle after
 * ps_orb_stereo_match_pair.  The work is ordered behind everything queued on the extractor's own stream, and what is queued on
 * that stream afterwards (the next batch) behind it; a batch run on a caller's stream is the caller's to order.  The kernel clamps
 * n[k] to the device-side count; if the two differ the frame is marked, and the next call that consumes it fails with
 * PS_ERR_INVALID.  The keypoints are the extractor's (mvKeys): they equal mvKeysUn only for rectified input (DistCoef == 0,
 * Frame::UndistortKeyPoints src/Frame.cc:2039-2044 - every configuration of BASELINE.md). */
int ps_frame_publish_orb(ps_frame* const* frames, int nframes, ps_orb* h, const int32_t* image, const int32_t* pair, const int32_t* n,
                         float min_x, float min_y, float grid_w_inv, float grid_h_inv);
/* Keypoints of the last publish (as the publisher stated them). */
int ps_frame_count(ps_frame* f, int* n);
/* GPU time of the last publish into the handle, upload included (HIP events on the publishing stream; blocks until it is done). */
int ps_frame_last_publish_ms(ps_frame* f, float* ms);
/* Test access (blocking).  what: 0 x, 1 y, 2 octave, 3 angle, 4 u_right (n x 4 bytes each), 5 descriptors (n x 32),
 * 6 cell_off (64 * 48 + 1 int32), 7 cell_idx (n int32: the lists, then zeros for keypoints outside the grid).  *n = keypoints. */
int ps_frame_debug_read(ps_frame* f, int what, void* out, size_t out_bytes, int* n);
/* ps_search_by_projection / ps_fuse_search with the train side of problem p taken from frames[p] where that is non-null:
 * x, y, octave, angle, u_right, desc, cell_off, cell_idx and the four grid parameters of probs[p].train are then ignored (they
 * may be NULL) and train.n must equal the handle's count (else PS_ERR_INVALID).  occupied, in_bbox and match_of_train stay host
 * arrays: they change from call to call.  frames[p] == NULL: the problem is served from its host arrays as in the plain call;
 * a batch may mix both kinds, and one handle may back several problems.  Everything else - the wide re-run, the per-problem
 * capacity failure, ps_matcher_last_kernel_ms - is that of the plain calls. */
int ps_search_by_projection_frames(ps_matcher* m, ps_proj_problem* probs, ps_frame* const* frames, int nprob);
int ps_fuse_search_frames(ps_matcher* m, ps_fuse_problem* problems, ps_frame* const* frames, int nproblems);

/* LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:414-707) for a batch of independent keyframes, each with its ordered
 * neighbours: ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:783-979, called at LocalMapping.cc:496) against every
 * neighbour, then the triangulation of every match and its gates (LocalMapping.cc:461-475, :519-684).
 *
 * ps_tri_keyframe is one KeyFrame as both halves read it: x, y, octave, angle = mvKeysUn; x_raw, y_raw = mvKeys[i].pt, which
 * KeyFrame::UnprojectStereo reads (src/KeyFrame.cc:716-717; NULL = the same as x, y); u_right, depth = mvuRight, mvDepth
 * (u_right >= 0 implies depth > 0); desc = mDescriptors rows; node[i] = the id of the mFeatVec node that lists feature i, -1
 * for a feature in none; occupied[i] = GetMapPoint(i) != NULL; rcw (row-major), tcw, ow = GetRotation, GetTranslation,
 * GetCameraCenter; fx .. mbf the members of that name; scale_factors, level_sigma2 = mvScaleFactors, mvLevelSigma2.
 * f12[i] = ComputeF12(kf1, kf2[i]) row-major (LocalMapping.cc:804-823): host glue, the caller's.
 *
 * The winner rule.  The candidates of feature idx1 are the unoccupied features of the neighbour with the same node id (under
 * only_stereo: the stereo ones), in ascending index - the order DBoW2::FeatureVector::addFeature builds.  vbMatched2
 * (ORBmatcher.cc:803) is read at :852 and never written, so idx1's partner depends on no other feature, and one feature of the
 * neighbour may be chosen by several.  No gate (:865-877: TH_LOW, the epipole disc for mono-mono pairs, CheckDistEpipolarLine
 * :261-278) depends on bestDist, and `dist > bestDist` (:865) lets an equal distance replace the held one: the winner is the
 * least distance <= 50 among the candidates that pass the gates, and among equal distances the HIGHEST index.
 * check_orientation applies the 30-bin histogram and ComputeThreeMaxima (:890-936) to the matches of one neighbour.
 *
 * The chain rule.  The only state the reference carries from one neighbour to the next is pKF1->GetMapPoint(idx1) (:826-830),
 * filled by mpCurrentKeyFrame->AddMapPoint(pMP, idx1) (LocalMapping.cc:693) when a match passes every gate.  With chain = 1
 * neighbour i sees kf1.occupied OR "status 0 at an earlier neighbour": such a feature is skipped - status 2, no match, no
 * histogram entry - which equals the reference's sequential loop.  chain = 0 serves every neighbour from kf1.occupied alone
 * (SearchForTriangulation by itself).  CheckNewKeyFrames()'s early return (LocalMapping.cc:455) is not modelled, like the
 * abort flag of ps_local_ba_batch.  pKF2->AddMapPoint (:694) fills a slot of a neighbour, which no later search of the same
 * call reads as long as the neighbours are distinct keyframes.
 *
 * triangulate = 1 restates LocalMapping.cc:461-475 and :519-684 for a stereo / RGB-D system (!mbMonocular): a neighbour whose
 * baseline is below its mb is skipped as a whole (status 11 everywhere, nmatches 0); otherwise every surviving match gets the
 * rays and cosParallaxRays, cosParallaxStereo1 / 2 (the `if / else if` of :552-555), the three-way choice between linear
 * triangulation, UnprojectStereo(idx1) and UnprojectStereo(idx2), the depth tests, the reprojection tests (5.991 / 7.8, with
 * mpCurrentKeyFrame->mbf for both keyframes as written at :631, :658) and the distance-ratio test against ratio_factor
 * (1.5f * mfScaleFactor).  Float expressions are evaluated as written; cv::Mat products, Mat::dot and cv::norm accumulate in
 * double and round once.  Two modelling choices, where the reference's arithmetic is OpenCV- or libm-internal:
 *   - the null vector: cv::SVD::compute on the 4 x 4 float matrix A (:576) becomes the right singular vector of the least
 *     singular value computed in FP64 on the float entries of A (one-sided Jacobi); the division by its fourth component is
 *     FP64, each coordinate is rounded to float once; "w == 0" tests the fourth component rounded to float;
 *   - the cosine: cos(2 * atan2(mb / 2, depth)) (:553, :555) is evaluated in FP64 on the float mb / 2 and depth, rounded once.
 *
 * Outputs, per neighbour i and feature idx1 of keyframe 1 ([k][n1] row-major):
 *   match    : idx2 or -1 - vMatches12 after the rotation check (and, with chain, without the skipped features)
 *   nmatches : [k] the return value of SearchForTriangulation
 *   status   : (triangulate) 0 point created, 1 no match, 2 the slot of keyframe 1 is occupied at this neighbour, 3 low
 *              parallax (:595), 4 w == 0 (:580), 5 z1 <= 0, 6 z2 <= 0, 7 reprojection in keyframe 1, 8 reprojection in the
 *              neighbour, 9 zero distance (:674), 10 scale ratio (:683), 11 neighbour skipped by the baseline gate
 *   x3d      : (triangulate) [k][n1][3], the new point where status is 0
 *   nnew     : points created over all neighbours (the reference's nnew)
 * With triangulate = 0, x3d and status are not written and may be NULL.  What follows a created point - new MapPoint,
 * AddObservation, AddMapPoint, ComputeDistinctiveDescriptors, UpdateNormalAndDepth, mlpRecentAddedMapPoints (:688-704) - is
 * map surgery and stays with the caller, in (neighbour, idx1) order.
 *
 * Limits: n <= 8191 features per keyframe, k <= 32 neighbours.  A problem beyond them fails alone: its outputs are left
 * untouched and the call returns PS_ERR_CAPACITY after serving the others.  n1 == 0, k == 0 and a neighbour with n == 0 are
 * valid and give empty results.  A node may hold any number of features. */
typedef struct ps_tri_keyframe {
  int32_t n;
  const float* x; const float* y;
  const float* x_raw; const float* y_raw;
  const int32_t* octave; const float* angle;
  const float* u_right; const float* depth;
  const uint8_t* desc;                 /* [n][32] */
  const int32_t* node;
  const uint8_t* occupied;
  float rcw[9], tcw[3], ow[3];
  float fx, fy, cx, cy, invfx, invfy, mb, mbf;
  float scale_factors[8], level_sigma2[8];
} ps_tri_keyframe;
typedef struct ps_tri_problem {
  ps_tri_keyframe kf1;                 /* mpCurrentKeyFrame */
  int32_t k;                           /* neighbours, in vpNeighKFs order */
  const ps_tri_keyframe* kf2;          /* [k] */
  const float* f12;                    /* [k][9] */
  int32_t only_stereo, check_orientation, triangulate, chain;
  float ratio_factor;
  int32_t* match;                      /* out [k][n1] */
  int32_t* nmatches;                   /* out [k] */
  float* x3d;                          /* out [k][n1][3] */
  uint8_t* status;                     /* out [k][n1] */
  int32_t* nnew;                       /* out, one value */
} ps_tri_problem;
int ps_create_new_map_points(ps_matcher* m, ps_tri_problem* probs, int nprob);
/* ... with x, y, octave, angle, u_right and desc of keyframe 1 of problem p taken from kf1_frames[p] where that is non-null
 * (those six may then be NULL; x_raw / y_raw = NULL means the handle's x, y).  node, occupied, depth and the pose stay host
 * fields: they change from call to call.  kf1.n must equal the handle's count (else PS_ERR_INVALID); ordering and lifetimes
 * are those of ps_search_by_projection_frames.  The current keyframe is read once per neighbour, so it is published once and
 * read k times. */
int ps_create_new_map_points_frames(ps_matcher* m, ps_tri_problem* probs, ps_frame* const* kf1_frames, int nprob);

/* The loop-closure and relocalisation projection matchers: the four ORBmatcher members between the keyframe database and the
 * Sim3 / PnP solvers.  All are windowed Hamming searches of projected map points into a 64 x 48 feature grid; `train` is the side
 * being searched into, as ps_proj_train documents it (x, y, octave, angle, desc, the grid as CSR and its four parameters; u_right
 * and in_bbox are not read).  Both calls are batched over independent problems.
 *
 * ps_kf_search serves the three one-directional members, selected by `mode`:
 *   mode 0 : SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)              (src/ORBmatcher.cc:413-526, LoopClosing.cc:378)
 *            gates, in the reference's order: z < 0; KeyFrame::IsInImage (upper bounds exclusive, KeyFrame.cc:706-709); distance
 *            outside [0.8 min, 1.2 max]; PO.Pn < 0.5 dist.  PredictScale(dist, pKF), KeyFrame::GetFeaturesInArea(u, v, th *
 *            scale[level]), candidates of octave level-1 .. level, a slot with vpMatched[idx] != NULL is skipped, the first
 *            strict minimum in traversal order wins, accepted at <= TH_LOW, and vpMatched[bestIdx] = pMP is seen by every later
 *            point.  train.occupied[j] = vpMatched[j] != NULL at entry; q_valid[i] = !pMP->isBad() && !spAlreadyFound.count(pMP)
 *            (the set holds vpMatched at entry).  Out: match_of_train[n] = point index or -1 (slot left alone), nmatches.
 *   mode 1 : Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)                       (:1262-1385, LoopClosing.cc:602)
 *            the same gates and level window, no occupancy test and - unlike Fuse(KeyFrame*, vpMapPoints, th), which
 *            ps_fuse_search serves - no reprojection gate.  q_valid[i] = !isBad() && !pKF->GetMapPoints().count(pMP).
 *            Out, as ps_fuse_search: best_idx[nq] (-1 unless bestDist <= TH_LOW), best_dist[nq] (256 without a candidate);
 *            nmatches = the return value nFused.  Replace / AddObservation / AddMapPoint (:1369-1379) stay with the caller, in
 *            candidate order.
 *   mode 2 : SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)  (:2529-2656, Tracking.cc:3613, :3627)
 *            the queries are the keyframe's own slots: q_valid[i] = pMP && !isBad() && !sAlreadyFound.count(pMP), q_angle[i] =
 *            pKF->mvKeysUn[i].angle.  As written there: no depth-sign gate (a point behind the camera whose projection is in
 *            bounds is searched); u = ((fx * xc) * invzc) + cx; inclusive bounds; no viewing-angle gate;
 *            Frame::GetFeaturesInArea(u, v, r, level-1, level+1); a slot with mvpMapPoints[i2] != NULL is skipped (train.occupied,
 *            no Observations() test); accepted at <= th_dist (ORBdist: 100 and 64 in the reference), seen by later queries; the
 *            rotation histogram (check_orientation) uses factor = 1.0f / HISTO_LENGTH, so bins 0 .. 12 fill, before
 *            ComputeThreeMaxima.  Out: match_of_train[n] = query index, -1 left alone, -2 assigned and reset by the rotation
 *            check; nmatches.  A non-finite u or v (camera-frame z == 0) is undefined in the reference; here it is outside the
 *            image.
 * The pose is decomposed by the caller: rcw, tcw, ow = Rcw, tcw, Ow of :422-426 / :1271-1275 / :2533-2535 (host glue, like f12 of
 * ps_tri_problem; pointslot_amd/host/ORBmatcher.h and pointslot_amd.matcher.decompose_scw state one model of it).  bounds =
 * mnMinX, mnMaxX, mnMinY, mnMaxY; q_pos / q_normal / q_min_dist / q_max_dist / q_desc as in ps_fuse_problem (q_normal unused in
 * mode 2).  Float arithmetic as in ps_fuse_search: R X + t with the products and their sum in double, rounded once, then a float
 * add; cv::norm and Mat::dot in double; PredictScale = ceil(log((double)ratio) / (double)logScale) on the float ratio.
 *
 * ps_search_by_sim3 serves SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (:1387-1611, LoopClosing.cc:326).  A side is
 * a keyframe: its features (train) and per slot has_point = pMP && !pMP->isBad(), pos = GetWorldPos, min_dist / max_dist,
 * point_desc = pMP->GetDescriptor() (the point's, not the feature's row), already = vbAlreadyMatched1/2 (:1417-1427); rcw, tcw,
 * bounds, scale_factors, log_scale_factor, n_levels.  fx, fy, cx, cy are keyframe 1's and serve both directions, as written at
 * :1390-1393.  sr12, t12, sr21, t21 are :1404-1406, the caller's.  Each direction: p1 = R1w X + t1w, then p2 = sR21 p1 + t21 (two
 * rounded steps); gates z < 0, IsInImage of the other keyframe, norm(p2) outside [0.8 min, 1.2 max]; PredictScale with the other
 * keyframe's tables; levels level-1 .. level; accepted at <= TH_HIGH; no occupancy.  Then the agreement pass (:1595-1608).
 * Out: match12[n1] = idx2 where both directions agree, -1 elsewhere (also where already1: the caller keeps its pointer); nfound;
 * match1[n1] / match2[n2] = vnMatch1 / vnMatch2, either may be NULL.
 *
 * Limits: n <= 8191 features per searched side, nq <= 32768 points.  nq == 0, n == 0 and nprob == 0 are valid and give empty
 * results.  The order-dependent modes keep, per point, the candidates that can ever be taken (free at entry, within th_dist): a
 * point with more than 32 of them makes its problem run again with a store of 1024.  Only a problem beyond the limits or beyond
 * that store fails: its outputs are untouched, nmatches (nfound) = -1, and the call returns PS_ERR_CAPACITY after serving all
 * other problems.  Null pointers, a bad mode, n_levels outside 1 .. 8 or th_dist outside 0 .. 255: PS_ERR_INVALID.
 * The _frames variants take the searched side of problem p from frames[p] where that is non-null, with the semantics of
 * ps_search_by_projection_frames (occupied and the outputs stay host arrays; one handle may back several problems - a
 * relocalising frame is searched once per candidate keyframe).  For Sim3, frames1[p] / frames2[p] hold the features of keyframe
 * 1 / 2; either array may be NULL.  ps_matcher_last_kernel_ms covers these calls. */
typedef struct ps_kf_search_problem {
  ps_proj_train train;
  int32_t mode;              /* 0, 1, 2: see above */
  int32_t nq;
  const uint8_t* q_valid;
  const float* q_pos;        /* [nq][3] GetWorldPos() */
  const float* q_normal;     /* [nq][3] GetNormal(); modes 0, 1 */
  const float* q_min_dist;   /* mfMinDistance (the 0.8 / 1.2 factors are applied inside) */
  const float* q_max_dist;
  const uint8_t* q_desc;     /* [nq][32] GetDescriptor() */
  const float* q_angle;      /* mode 2 with check_orientation */
  float rcw[9], tcw[3], ow[3];
  float fx, fy, cx, cy;
  float bounds[4];
  float scale_factors[8];
  float log_scale_factor;
  int32_t n_levels;
  float th;
  int32_t th_dist;           /* mode 2: ORBdist; modes 0, 1 use TH_LOW */
  int32_t check_orientation; /* mode 2: mbCheckOrientation */
  int32_t* match_of_train;   /* out [train.n], modes 0, 2 */
  int32_t* best_idx;         /* out [nq], mode 1 */
  int32_t* best_dist;        /* out [nq], mode 1 */
  int32_t nmatches;          /* out */
} ps_kf_search_problem;
int ps_kf_search(ps_matcher* m, ps_kf_search_problem* probs, int nprob);
int ps_kf_search_frames(ps_matcher* m, ps_kf_search_problem* probs, ps_frame* const* frames, int nprob);

typedef struct ps_sim3_side {
  ps_proj_train train;
  const uint8_t* has_point;
  const float* pos;          /* [n][3] */
  const float* min_dist;
  const float* max_dist;
  const uint8_t* point_desc; /* [n][32] */
  const uint8_t* already;
  float rcw[9], tcw[3];
  float bounds[4];
  float scale_factors[8];
  float log_scale_factor;
  int32_t n_levels;
} ps_sim3_side;
typedef struct ps_sim3_problem {
  ps_sim3_side kf1, kf2;
  float fx, fy, cx, cy;      /* keyframe 1's */
  float sr12[9], t12[3], sr21[9], t21[3];
  float th;
  int32_t* match12;          /* out [kf1.train.n] */
  int32_t* match1;           /* out [kf1.train.n] or NULL */
  int32_t* match2;           /* out [kf2.train.n] or NULL */
  int32_t nfound;            /* out */
} ps_sim3_problem;
int ps_search_by_sim3(ps_matcher* m, ps_sim3_problem* probs, int nprob);
int ps_search_by_sim3_frames(ps_matcher* m, ps_sim3_problem* probs, ps_frame* const* frames1, ps_frame* const* frames2, int nprob);

/* ------------------------------------------------------------------------------------------------
 * Sim3Solver (src/Sim3Solver.cc) - the RANSAC over Horn's closed-form similarity between the two keyframes of a loop candidate.
 * One call evaluates every hypothesis of every problem of a batch; a problem is one candidate keyframe pair.  The call keeps no
 * state between invocations and is exact given the draws: what iterate() does sequentially (:141-208) is a walk over `inliers`.
 *   n, x3dc1 / x3dc2 [n][3] : mvX3Dc1 / mvX3Dc2, the matched points in the frame of camera 1 / 2 (:95-99)
 *   max_err1 / max_err2 [n] : mvnMaxError1 / 2 as floats.  They are std::vector<size_t> in the reference: 9.210 * sigma2 is
 *                             TRUNCATED to an integer before the float comparison (level 1 gates at 13, not 13.26)
 *   k1 / k2                 : fx, fy, cx, cy of keyframe 1 / 2
 *   fix_scale               : mbFixScale
 *   nhyp, draws [nhyp][3]   : per hypothesis the three raw rand() values (0 .. 2^31 - 1) its draw consumes.  Hypothesis h applies
 *                             DUtils::Random::RandomInt to them and draws without replacement from 0 .. n - 1 as :164-178 do
 *   min_inliers             : mRansacMinInliers
 *   inliers [nhyp]          : out, mnInliersi of every hypothesis
 *   model [nhyp][13]        : out, ms12i, mR12i row-major, mt12i.  A quaternion with a zero imaginary part gives NaN, as in the
 *                             reference (0 * (1 / 0)): the hypothesis has no inliers
 *   mask                    : out or NULL, nhyp x ceil(n / 64) words: bit (i & 63) of word (i >> 6) is mvbInliersi[i]
 *   first_success           : out, the smallest h with inliers[h] > min_inliers, else -1
 *   best                    : out, the last h that attains the running maximum (:184 compares with >=), -1 without hypotheses
 * Arithmetic: the float expressions as written; cv::Mat products, Mat::dot and cv::norm with products and sums in double, rounded
 * once; the eigenvector is that of the float32 N, computed in FP64, with q0 >= 0 (DESIGN.md 4j lists the readings).
 * Limits: n <= 32767, nhyp <= 4096; a problem beyond them fails alone (first_success = best = -2) and the call returns
 * PS_ERR_CAPACITY after the others are served.  A problem with nhyp == 0, n < min_inliers or n < 3 is legal, costs nothing and
 * leaves its arrays untouched (first_success = best = -1).  ps_matcher_last_kernel_ms covers the call. */
typedef struct ps_sim3_ransac_problem {
  int32_t n;
  const float* x3dc1;
  const float* x3dc2;
  const float* max_err1;
  const float* max_err2;
  float k1[4], k2[4];
  int32_t fix_scale;
  int32_t nhyp;
  const int32_t* draws;
  int32_t min_inliers;
  int32_t* inliers;
  float* model;
  uint64_t* mask;
  int32_t first_success;
  int32_t best;
} ps_sim3_ransac_problem;
int ps_sim3_ransac(ps_matcher* m, ps_sim3_ransac_problem* probs, int nprob);
/* Sim3Solver::SetRansacParameters (:115-139), host only: *iterations = mRansacMaxIts for n correspondences, with the float epsilon. */
int ps_sim3_ransac_iterations(double probability, int min_inliers, int max_iterations, int n, int* iterations);

/* ------------------------------------------------------------------------------------------------
 * Bag of words - the DBoW2 vocabulary the reference keeps as ORBVocabulary (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h with
 * FORB), Frame::ComputeBoW / KeyFrame::ComputeBoW (src/Frame.cc:2040-2047, src/KeyFrame.cc:114-123) and the two
 * ORBmatcher::SearchByBoW overloads (src/ORBmatcher.cc:280-410, :646-781).
 *
 * ps_vocabulary is an opaque, immutable tree in HBM, built once per device and read by any number of matcher handles on any
 * number of threads.  It has no stream of its own: the work of a call runs on the ps_matcher passed to it.  A vocabulary and a
 * matcher on different devices make the call return PS_ERR_INVALID.
 *
 * ps_vocabulary_create takes the records of the binary file in file order (loadFromBinaryFile, TemplatedVocabulary.h:1343-1384):
 * record i becomes node i + 1, the root is node 0; parent[i] is the record's parent id, desc[i] its 32-byte descriptor,
 * weight[i] its weight, is_leaf[i] != 0 makes it a word.  Children are listed in record order (children.push_back, :1368) and
 * word ids are assigned in order of the leaf records (:1372-1377).  Accepted: 1 <= k <= 20, 1 <= L <= 10, weighting 0 TF_IDF,
 * 1 TF, 2 IDF, 3 BINARY (BowVector.h), scoring 0 (L1_NORM) only.  k and L are recorded as the file states them; a node may have
 * any number of children and a leaf may sit at any depth, as in the reference.  Rejected with PS_ERR_INVALID - where the
 * reference runs into undefined behaviour: a parent id that does not precede its child (parent[i] < 0 or > i), a parent that is
 * a leaf, an inner node (the root included) with no children.
 *
 * ps_vocabulary_load_binary reads the layout the reference reads: u32 nb_nodes, u32 size_node (= 41), then k, L, scoring,
 * weighting as i32; nb_nodes records of i32 parent, 32 B descriptor, f32 weight, u8 leaf.  Exactly nb_nodes records are read
 * and the file must end there.  The reference's `while(!f.eof())` (:1361) makes one more pass over the stale buffer after the
 * last record and writes m_nodes[nb_nodes + 1], one past the vector: undefined behaviour, which is not modelled.  The parser is
 * host-only (csrc/vocab_file.h).  PS_ERR_INVALID: unreadable, truncated or inconsistent file. */
typedef struct ps_vocabulary ps_vocabulary;
int ps_vocabulary_create(int device, int k, int L, int scoring, int weighting, int nnodes, const int32_t* parent, const uint8_t* desc,
                         const float* weight, const uint8_t* is_leaf, ps_vocabulary** out);
int ps_vocabulary_load_binary(int device, const char* path, ps_vocabulary** out);
void ps_vocabulary_destroy(ps_vocabulary* v);
/* k, L as given; nodes = nnodes + 1 (the root included); words = leaf records.  Any pointer may be NULL. */
int ps_vocabulary_info(const ps_vocabulary* v, int32_t* k, int32_t* L, int32_t* nodes, int32_t* words);

/* TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup) (TemplatedVocabulary.h:1133-1200 over the
 * per-feature descent :1224-1265) for a batch of frames.  Per problem, in: n descriptors and levelsup; out:
 *   word[n]   : the WordId of feature i, -1 for a stopped word
 *   node[n]   : the NodeId met at level L - levelsup on the way down, the root 0 when that level is <= 0 (:1233), -1 for a stopped
 *               word - exactly what ps_tri_keyframe.node and ps_bow_side.node take; the FeatureVector is node -> features in
 *               ascending feature order (addFeature's order)
 *   bow_id[], bow_val[], bow_n : the BowVector, ids ascending as std::map iterates, values double; room for n entries each
 * The descent takes the first child of least Hamming distance (`d < best_d` is strict, :1250: on ties the earliest child wins)
 * until it stands on a leaf.  A word of weight <= 0 is stopped (:1163, :1191): it appears in neither vector.  TF_IDF and TF sum
 * the weights per word (addWeight), IDF and BINARY keep the first (addIfNotExist); the L1 normalisation of BowVector.cpp:62-84
 * follows (the sum of |values| is formed in an order of the kernel's own; skipped when it is not > 0).
 * Modelling choice: a leaf shallower than level L - levelsup leaves *nid unwritten in the reference (:1257 never fires), so
 * its callers read an uninitialised local; here node is then that leaf's own id.
 * Limits: n <= 8191 per problem; a problem beyond that fails alone (bow_n = -1, outputs untouched) and the call returns
 * PS_ERR_CAPACITY after serving the others.  n == 0 is valid. */
typedef struct ps_bow_problem {
  int32_t n;
  const uint8_t* desc;   /* [n][32] */
  int32_t levelsup;
  int32_t* word;         /* out [n] */
  int32_t* node;         /* out [n] */
  int32_t* bow_id;       /* out [<= n] */
  double* bow_val;       /* out [<= n] */
  int32_t bow_n;         /* out */
} ps_bow_problem;
int ps_bow_transform(ps_matcher* m, const ps_vocabulary* v, ps_bow_problem* probs, int nprob);

/* ORBmatcher::SearchByBoW, both overloads, batched.  Side a is pKF / pKF1, side b is F / pKF2:
 *   n, desc = mDescriptors rows; angle: see the modes; node[i] = the id of the mFeatVec node that lists feature i (-1: none -
 *   ps_bow_transform's node[]); has_point[i] = pMP && !pMP->isBad() for the side's GetMapPointMatches()[i].
 * Common rules.  The features of a node are taken in ascending index on both sides (mFeatVec's order); only nodes present on
 * both sides are searched (:302-386, :676-758); a feature of side a without a point is skipped.  `dist<bestDist1` (:338, :712)
 * makes the first admitted candidate of least distance the best; bestDist2 ends as the least distance over all other admitted
 * candidates (256 if none), so an equal distance makes the ratio test fail for nn_ratio <= 1.  The ratio test
 * (float)bestDist1 < nn_ratio * (float)bestDist2 is in float as written.  check_orientation applies the 30-bin histogram
 * (round(rot * 30 / 360), bin 30 -> 0) and ComputeThreeMaxima to the accepted matches.
 *   mode 0 (KeyFrame*, Frame&, :280-410): a candidate of b is admitted unless an earlier feature of a has taken it
 *     (vpMapPointMatches[realIdxF], :331 - a feature sits in one node only, so only the order within the node matters); accepted
 *     when bestDist1 <= 50; match is [b.n] and holds the index into a (the MapPoint of pKF the reference stores), -1 = NULL;
 *     b.has_point is ignored (may be NULL); a.angle = pKF->mvKeysUn, b.angle = F.mvKeys (:356-360).
 *   mode 1 (KeyFrame*, KeyFrame*, :646-781): a candidate needs b.has_point and must not be in vbMatched2 (:702); accepted when
 *     bestDist1 < 50 - strict, unlike mode 0; match is [a.n] and holds the index into b; both angles are mvKeysUn.
 * nmatches is the return value.  Limits: n <= 8191 per side; a problem beyond that fails alone (nmatches = -1, match untouched)
 * and the call returns PS_ERR_CAPACITY after serving the others.  Empty sides and disjoint node sets are valid and give
 * empty results. */
typedef struct ps_bow_side {
  int32_t n;
  const uint8_t* desc;       /* [n][32] */
  const float* angle;
  const int32_t* node;
  const uint8_t* has_point;
} ps_bow_side;
typedef struct ps_bow_search_problem {
  ps_bow_side a, b;
  int32_t mode;
  float nn_ratio;
  int32_t check_orientation;
  int32_t* match;            /* out: mode 0 [b.n], mode 1 [a.n] */
  int32_t nmatches;          /* out */
} ps_bow_search_problem;
int ps_search_by_bow(ps_matcher* m, ps_bow_search_problem* probs, int nprob);

/* ------------------------------------------------------------------------------------------------
 * Keyframe database - KeyFrameDatabase (src/KeyFrameDatabase.cc:41-310): add, erase, clear, DetectLoopCandidates and
 * DetectRelocalizationCandidates, and the `mpORBVocabulary->score` of LoopClosing::DetectLoop's minScore loop
 * (src/LoopClosing.cc:127-141, Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68).  It turns the BowVectors ps_bow_transform
 * writes into the candidate keyframes ps_search_by_bow is then run over.
 *
 * ps_kfdb is an opaque, mutable store in HBM: one row of word ids and one row of values per keyframe (a forward store; the
 * reference's inverted file is not kept).  Like ps_vocabulary it has no stream of its own: add, query and score run on the
 * ps_matcher passed to them and return when the work is done.  A database and a matcher on different devices make the call
 * return PS_ERR_INVALID.  Calls on one database are serialised.
 *
 * ps_kfdb_create: capacity = the number of live keyframes it can hold, 1 .. 4096; max_words = the longest BowVector it
 * stores, 1 .. 8191.  It takes capacity * roundup(max_words, 64) * 12 bytes of device memory.
 * ps_kfdb_add stores n keyframes under caller-chosen ids.  bow_id[e] / bow_val[e] / bow_n[e] are entry e's BowVector exactly
 * as ps_bow_transform writes it: ids ascending, values double.  bow_n[e] == 0 is valid: such a keyframe can never be found.
 * PS_ERR_INVALID, nothing stored: a null or negative argument, ids of a vector not strictly ascending or negative, an id that is
 * already stored or appears twice in the call (the reference would list such a keyframe twice and count its words double: not
 * modelled).  An entry with more than max_words words, and an entry for which no room is left, fails alone: the call returns
 * PS_ERR_CAPACITY after storing the others.  stored (may be NULL) receives 1 per stored entry, 0 per failed one.  A database
 * takes 2^32 - 1 adds between two ps_kfdb_clear; further ones fail with PS_ERR_CAPACITY.
 * ps_kfdb_erase removes the named keyframes; unknown ids are ignored, as in the reference's loop (:59-66).  ps_kfdb_clear
 * removes all.  ps_kfdb_size: the number of live keyframes.
 *
 * ps_kfdb_query serves a batch of queries up to the scored sharing list (:79-140, :202-254).  Per problem, in: the query's
 * BowVector (n <= 8191, ids strictly ascending), mode 0 = DetectRelocalizationCandidates, 1 = DetectLoopCandidates, and for mode 1
 * excluded[nexcluded] = the ids of pKF->GetConnectedKeyFrames() (ids that are not stored are ignored).  Out, with room for
 * ps_kfdb_size entries each:
 *   share_id[], nshare : lKFsSharingWords in the reference's order.  Its walk goes over the query's words in ascending id and,
 *                  inside a word's list, in push_back order, and lists a keyframe where it meets it first: a keyframe's place is
 *                  the pair (least word it has in common with the query, its add order).  erase keeps the order of the others; a
 *                  keyframe erased and added again goes to the back.  In mode 1 an excluded keyframe is never listed and takes
 *                  no part in maxCommonWords (:97-101).
 *   share_words[]    : mnRelocWords / mnLoopWords, the number of common words
 *   min_common_words : `int minCommonWords = maxCommonWords*0.8f` - the int-to-float product, truncated (0 for an empty list)
 *   share_score[]    : a keyframe is scored when words > min_common_words: (float)score(query, keyframe), L1Scoring::score with
 *                  the query as v1 - the double sum of fabs(vi - wi) - fabs(vi) - fabs(wi) over the common words in ascending
 *                  word id, one addition after the other, then -score/2.0, rounded to float once.
 *                  mode 1: that score where words > min_common_words, 0 elsewhere (mLoopScore is only read behind that test).
 *                  mode 0: the keyframe's reloc_score after this query - fresh for the scored keyframes, stale for the others.
 * Modelling choice (reloc_score).  KeyFrame's constructor does not initialise mRelocScore (KeyFrame.cc:43), and the covisibility
 * stage of DetectRelocalizationCandidates adds it for every neighbour that shares a word (:274-277), scored by this query or
 * not: it reads what the last earlier relocalisation query wrote, or indeterminate memory.  The database keeps one reloc_score
 * float per stored keyframe: 0.0f at add, written whenever a mode-0 query scores the keyframe, kept from query to query and
 * from call to call.  The queries of one call are served in array order with respect to it: the results do not depend on how
 * the queries are split over calls.
 * A problem with n > 8191 fails alone (nshare = -1, outputs untouched) and the call returns PS_ERR_CAPACITY after serving the
 * others.  An empty query and an empty database give nshare = 0.  At most 65535 problems per call.
 *
 * ps_kfdb_score: out[i] = L1Scoring::score(query, stored keyframe ids[i]) in double, the same ordered sum.  An unknown id gives
 * NaN in its place and the call returns PS_ERR_INVALID after writing the others.
 *
 * ps_kfdb_select is the covisibility stage (:145-197, :259-309) over the lists of one query.  It is a host-only function: no
 * device, no handle.  neigh[i*10 .. i*10 + neigh_n[i]) are the ids of share_id[i]->GetBestCovisibilityKeyFrames(10), in its order;
 * they are read only for the entries with share_words[i] > min_common_words (neigh_n may be anything elsewhere).  All arithmetic
 * is float.  mode 1: the entries with share_score >= min_score are retained; a neighbour contributes when it is in the list with
 * words > min_common_words; bestAccScore starts at min_score.  mode 0 (min_score is ignored): every scored entry is retained; a
 * neighbour contributes when it is in the list at all, with its share_score; bestAccScore starts at 0.  Both: accScore >
 * bestAccScore and neighbour score > bestScore are strict; an entry's pBestKF becomes a candidate when its accScore > 0.75f *
 * bestAccScore; a pBestKF already among the candidates is dropped, the first occurrence keeps its place.  cand_out has room for
 * nshare ids.  PS_ERR_INVALID: a null argument, a neigh_n outside 0 .. 10 where it is read. */
typedef struct ps_kfdb ps_kfdb;
int ps_kfdb_create(int device, int capacity, int max_words, ps_kfdb** out);
void ps_kfdb_destroy(ps_kfdb* db);
int ps_kfdb_add(ps_kfdb* db, ps_matcher* m, const int64_t* ids, const int32_t* const* bow_id, const double* const* bow_val,
                const int32_t* bow_n, int n, int32_t* stored);
int ps_kfdb_erase(ps_kfdb* db, const int64_t* ids, int n);
int ps_kfdb_clear(ps_kfdb* db);
int ps_kfdb_size(const ps_kfdb* db, int32_t* size);
typedef struct ps_kfdb_query_problem {
  int32_t n;                 /* the query's BowVector */
  const int32_t* bow_id;
  const double* bow_val;
  int32_t mode;              /* 0 relocalisation, 1 loop */
  int32_t nexcluded;         /* mode 1 */
  const int64_t* excluded;
  int64_t* share_id;         /* out [ps_kfdb_size] */
  int32_t* share_words;      /* out [ps_kfdb_size] */
  float* share_score;        /* out [ps_kfdb_size] */
  int32_t nshare;            /* out */
  int32_t min_common_words;  /* out */
} ps_kfdb_query_problem;
int ps_kfdb_query(ps_kfdb* db, ps_matcher* m, ps_kfdb_query_problem* probs, int nprob);
int ps_kfdb_score(ps_kfdb* db, ps_matcher* m, const int32_t* bow_id, const double* bow_val, int bow_n, const int64_t* ids, int n,
                  double* out);
int ps_kfdb_select(int mode, float min_score, const int64_t* share_id, const int32_t* share_words, const float* share_score,
                   int nshare, int min_common_words, const int64_t* neigh, const int32_t* neigh_n, int64_t* cand_out, int32_t* ncand);


/* ------------------------------------------------------------------------------------------------
 * Optimiser — replaces the hot static members of ORB_SLAM2::Optimizer
 * (/root/reference/include/Optimizer.h:51-61, src/Optimizer.cc:249-1075) and the g2o solver stack they
 * instantiate.  All arithmetic is FP64 on float32 inputs, as in the reference.
 * SE3 poses cross this boundary either as the float 4x4 row-major matrix the reference keeps in
 * cv::Mat (Frame::mTcw) or as 7 doubles (tx,ty,tz,qx,qy,qz,qw) = g2o::SE3Quat::toVector().
 * ---------------------------------------------------------------------------------------------- */
typedef struct ps_optimizer ps_optimizer;
int ps_optimizer_create(int device, ps_optimizer** out);
void ps_optimizer_destroy(ps_optimizer* m);
/* GPU time of the last batch's kernel(s), from HIP events on the handle's stream. */
int ps_optimizer_last_kernel_ms(const ps_optimizer* m, float* ms);
/* Optional per-LM-iteration log (chi2, lambda, trials) of the next batches; for parity tests. */
int ps_optimizer_enable_trace(ps_optimizer* m, int enable);
int ps_optimizer_get_trace(const ps_optimizer* m, int problem, double* chi2_lambda_trials, int cap, int* n);

/* Converter::toSE3Quat / Converter::toCvMat (src/Converter.cc:37-71) for callers without Eigen. */
int ps_se3_from_mat4f(const float* m16, double* pose7);
int ps_se3_to_mat4f(const double* pose7, float* m16);

/* Optimizer::PoseOptimization(Frame*) (Optimizer.cc:249-477) for a batch of independent frames.
 *   n          : pFrame->N
 *   xw         : [n][3] world position of mvpMapPoints[i] (float, MapPoint::GetWorldPos)
 *   obs        : [n][3] mvKeysUn[i].pt.x, .pt.y, mvuRight[i] (uR < 0 => monocular edge)
 *   inv_sigma2 : [n]    mvInvLevelSigma2[mvKeysUn[i].octave]
 *   valid      : [n]    1 iff mvpMapPoints[i] != NULL
 *   fx..bf     : Frame::fx, fy, cx, cy, mbf
 *   tcw        : in: pFrame->mTcw; out: the pose passed to pFrame->SetPose
 *   outlier    : [n] in/out pFrame->mvbOutlier (entries with valid == 0 are left untouched)
 *   result     : out, the return value: nInitialCorrespondences - nBad, 0 when < 15 correspondences */
typedef struct ps_pose_problem {
  int32_t n;
  const float* xw; const float* obs; const float* inv_sigma2; const uint8_t* valid;
  float fx, fy, cx, cy, bf;
  float tcw[16];
  uint8_t* outlier;
  int32_t result;
} ps_pose_problem;
int ps_pose_optimize_batch(ps_optimizer* m, ps_pose_problem* probs, int nprob);

/* Optimizer::CFSE3ObjStateOptimization(Frame*, vnNeedToBeOptimized, verbose) (Optimizer.cc:479-753):
 * k objects of one frame optimised as ONE graph (k <= 16).  Object o owns the feature range
 * [off[o], off[o+1]) of the concatenated arrays.
 *   xo         : MapObjectPoint::GetInObjFramePosition (object-frame coordinates)
 *   obs        : mvObjKeysUn[o][j].pt.x, .pt.y, mvuObjKeysRight[o][j]
 *   valid      : 1 iff mvpMapObjectPoints[o][j] != NULL
 *   poses7     : in: MapObject::GetCFInFrameObjState(frame).pose (Tco); out: the optimised vertex
 *                estimate.  The translation of the input is also the measurement of the
 *                EdgeTransConstraintFromDetction prior (information 50 I).
 *   outlier    : in/out mvbObjKeysOutlier
 *   result     : out, 1 (true) / 0 (false: no object or fewer than 15 edges) */
typedef struct ps_cfse3_problem {
  int32_t k;
  const int32_t* off;
  const float* xo; const float* obs; const float* inv_sigma2; const uint8_t* valid;
  float fx, fy, cx, cy, bf;
  double* poses7;
  uint8_t* outlier;
  int32_t result;
} ps_cfse3_problem;
int ps_cfse3_optimize_batch(ps_optimizer* m, ps_cfse3_problem* probs, int nprob);

/* Optimizer::ObjectLocalBundleAdjustment(ObjectKeyFrame*, verbose) (Optimizer.cc:755-1075) on a graph the
 * caller has already collected (:755-818, :827-951 map 1:1 onto these arrays), for a batch of objects.
 *   poses7     : [np][7] in: Converter::toSE3Quat(pKFi->GetPose()) of the local (free) and fixed object
 *                keyframes; out: the optimised estimates (written back with pKF->SetPose, :1033-1064)
 *   pose_flags : [np] bit 0 = setFixed(true) (mnId == 0 or a lFixedCameras entry), bit 1 = VertexSE3Fix with
 *                whether_fixrollpitch (every local keyframe, :834-846); at most 128 free poses
 *   points     : [nl][3] in: MapObjectPoint::GetInObjFrameEigenPosition; out: SetInObjFramePosition (:1066-1074)
 *   e_*        : one entry per (point, observing keyframe): vertex indices, (u, v, uR) with uR < 0 for a
 *                monocular edge, mvInvLevelSigma2[octave]; at most one edge per (pose, point) pair
 *   erase      : [ne] out, 1 where the reference queues (pKFi, pMP) into vToErase (:988-1012)
 *   iterations / trials : out, LM iterations and damping trials executed (optimize(5) + optimize(10))
 *   trace      : NULL or room for 40 x 3 doubles: (chi2, lambda, trials) per LM iteration; n_trace = count */
typedef struct ps_ba_problem {
  int32_t np, nl, ne;
  double* poses7; const uint8_t* pose_flags;
  double* points;
  const int32_t* e_pose; const int32_t* e_point; const float* e_obs; const float* e_inv_sigma2;
  float fx, fy, cx, cy, bf;
  uint8_t* erase;
  int32_t n_erased, iterations, trials, n_trace;
  double* trace;
} ps_ba_problem;
int ps_object_ba_batch(ps_optimizer* m, ps_ba_problem* probs, int nprob);
/* The reprojection test of Tracking::DynamicStaticDiscrimination (src/Tracking.cc:2099-2181) for a batch of
 * tracked detections: every object point is moved as if the object were static, Pc = Tcw_cur * Tcw_last^-1 * (Tco_last * Po),
 * and its chi-square against the current observation is collected per kind (monocular: u_right < 0 / stereo); each list is
 * sorted, values above 5 x median dropped, the rest averaged in sorted order (FP64, bit-identical to the CPU statement).
 * The caller keeps the gates around it (depth range, image prior, :2082-2097) and feeds the averages to
 * DetectionObject::SetDynamicFlag(mono_avg, stereo_avg).  Poses are (tx, ty, tz, qx, qy, qz, qw). */
typedef struct ps_dyn_problem {
  int32_t n;                      /* mvpMapObjectPoints[order].size(), <= 2048 */
  const uint8_t* valid;           /* vMOPs[j] != NULL */
  const double* po;               /* [n][3] GetInObjFrameEigenPosition() */
  const float* obs;               /* [n][3] mvObjKeysUn[order][j].pt.x, .pt.y, mvuObjKeysRight[order][j] */
  const float* inv_sigma2;        /* [n] mvInvLevelSigma2[octave] */
  double last_tco[7];             /* pMO->GetCFInFrameObjState(mLastFrame.mnId).pose */
  double last_tcw[7], cur_tcw[7]; /* mLastFrame.mSETcw, mCurrentFrame.mSETcw */
  double fx, fy, cx, cy;          /* mdCamProjMatrix */
  float mbf;
  double mono_avg, stereo_avg;    /* out: monoDynaValAvg, stereoDynaValAvg (0 with fewer than 5 points of the kind) */
  int32_t mono_n, stereo_n;       /* out: monoPointNum, stereoPointNum after the rejection */
} ps_dyn_problem;
int ps_dynamic_discrimination_batch(ps_optimizer* h, ps_dyn_problem* problems, int nproblems);

/* Optimizer::LocalBundleAdjustment(KeyFrame*, pbStopFlag, Map*) (Optimizer.cc:1077-1417) on a collected
 * graph: same edge types and LM schedule with plain VertexSE3Expmap keyframes (pose_flags bit 1 = 0; bit 0 = fixed for
 * mnId == 0 and the fixed cameras) and world-frame map points.  The abort flag of the reference is not modelled. */
int ps_local_ba_batch(ps_optimizer* m, ps_ba_problem* probs, int nprob);

/* ------------------------------------------------------------------------------------------------
 * Lockstep tracker — the tracking thread's per-frame chain for many independent stereo sequences, resident on the device:
 *   Frame::Frame (ExtractORB x 2, ComputeStereoMatches, AssignFeaturesToGrid)      /root/reference/src/Frame.cc:709-722,1636-1656
 *   StereoInitialization / UpdateLastFrame / TrackWithMotionModel / TrackLocalMap   src/Tracking.cc:2840-3160
 *   (SearchByProjection(cur, last, th) with its 2 th retry, PoseOptimization, isInFrustum, SearchByProjection(F, points),
 *   PoseOptimization) and the constant-velocity model, src/Tracking.cc:1260-1286
 * in localisation mode (mbOnlyTracking), exactly the slice pointslot_amd/host/StereoOdometry.h drives through the calls
 * above — but queued on ONE stream per step with nothing returning to the host: no packing, no PCIe traffic besides the
 * images.  Independent sequences are the unit of parallelism (BASELINE config 4 / SURVEY.md 8e).  Results are identical to
 * the per-call driver's.  A handle is not re-entrant; several handles may run on several threads / streams side by side.
 * ---------------------------------------------------------------------------------------------- */
typedef struct ps_tracker ps_tracker;
typedef struct ps_tracker_config {
  int32_t n_sequences;               /* sequences advanced by one call                                         */
  int32_t width, height;             /* image size (all sequences share the rig)                               */
  float fx, fy, cx, cy, bf;          /* Camera.fx .. Camera.bf of the settings file                            */
  float th_depth;                    /* ThDepth (35 in the KITTI settings)                                     */
  int32_t nfeatures; float scale_factor; int32_t nlevels, ini_th_fast, min_th_fast;   /* ORBextractor.*      */
  int32_t max_steps;                 /* frames per sequence the handle keeps results for                       */
  int32_t device;
  int32_t max_objects;               /* detections per frame (SLOT.MODE 4 object chain; 0 = camera only, <= 16) */
  int32_t max_map_objects;           /* MapObjects a sequence can hold over its life (Tracking's AllObjects; the reference's list is
                                        unbounded, the device table is not): 0 = 8, <= 64.  A detection that would need one more is
                                        ignored and ps_tracker_fetch_objects reports PS_ERR_CAPACITY                            */
} ps_tracker_config;
/* what Tracking::Track leaves per frame and sequence */
typedef struct ps_track_stat {
  int32_t state;          /* 0 NOT_INITIALIZED, 1 OK, 2 LOST after the frame                                   */
  int32_t tracked;        /* the frame has a pose                                                              */
  int32_t n;              /* keypoints of the left image                                                       */
  int32_t mm_matches;     /* SearchByProjection(cur, last): matches of the attempt that was used               */
  int32_t retried;        /* the 2 * th retry ran (Tracking.cc:3042-3048)                                      */
  int32_t matches;        /* after the first PoseOptimization and the outlier discard (Tracking.cc:3062-3082)  */
  int32_t map_matches;    /* ... of which on map points with observations                                      */
  int32_t lm_candidates;  /* local-map points that passed Frame::isInFrustum                                   */
  int32_t lm_inliers;     /* mnMatchesInliers of TrackLocalMap                                                 */
  int32_t overflowed;     /* search windows of this frame that held more than 256 candidates: the matcher's candidate store is
                             bounded here (the reference's GetFeaturesInArea is not), candidates beyond it were not considered and
                             the frame's result may differ from the reference's; the other sequences are unaffected            */
  int32_t reserved[2];
} ps_track_stat;
int ps_tracker_create(const ps_tracker_config* cfg, ps_tracker** out);
void ps_tracker_destroy(ps_tracker* t);
/* One stereo frame of every sequence.  _device: images already in HBM, sequence k's left image at d_imgs + 2k * image_pitch,
 * its right image one pitch further, rows `stride` bytes apart.  The host form takes one pointer per image (asynchronous when
 * they come from ps_pinned_alloc).  Both return as soon as the step is queued. */
int ps_tracker_step_device(ps_tracker* t, const uint8_t* d_imgs, int stride, size_t image_pitch);
int ps_tracker_step(ps_tracker* t, const uint8_t* const* left, const uint8_t* const* right, int stride);
/* SLOT.MODE 4 (offline detections + instance masks), the whole of Tracking::Track's per-frame work: the camera chain above on the
 * background keypoints (Frame::AssignFeatures, src/Frame.cc:762-977: keypoints on mask != 0 leave the static set) and behind it
 * the object chain on the device -
 *   Frame::ExtractObjORB (cv::ORB(1000, 1.2, 8, 19) under the object masks, :2623-2665) and ComputeObjStereoMatches (:2318-2503),
 *   TrackMapObject (pose prediction, InitializeCurrentObjPose's RANSAC centroid, FineTuningUsing2dBox, MapObjectInit;
 *   src/Tracking.cc:1533-1930), TrackLastFrameObjectPoint (temporal points, SearchByBruceMatching, CFSE3ObjStateOptimization,
 *   :2288-2466), TrackObjectLocalMap (isInFrustum(pMP, nOrder), SearchByProjection(F, nOrder, MOPs), CFSE3, :2468-2712), the end of
 *   Track (MapObjectReInit for an object whose tracking failed, :1443-1478,1932-2031)
 * - in the localisation-mode slice pointslot_amd/object_tracker.py documents (an object's local map is the object keyframe of its
 * (re-)initialisation).  d_masks: per sequence the LEFT 8-bit id mask of Frame::ReadKittiSegmentationImage (0 background, 255
 * ignored, instance + 1), sequence k at d_masks + k * mask_pitch; d_dets: [n_sequences][max_objects] detections of the frame in
 * label order, unused slots with id < 0 behind the used ones.  Both in HBM; they must stay unchanged until the step has run.
 * (Environment, read at ps_tracker_create: PS_TRK_OVERLAP=1 runs ExtractObjORB on a second stream beside the camera chain - same
 * results; PS_TRK_DEBUG_SYNC=1 waits after every launch group and reports it on stderr.) */
typedef struct ps_detection {
  int32_t id;            /* DetectionObject::mnObjectID (the label's track id); < 0: empty slot                               */
  int32_t bbox[4];       /* mrectBBox: x, y, width, height (cv::Rect of the label's truncated doubles)                         */
  int32_t reserved[3];
  double scale[3];       /* mScale: length, height, width                                                                      */
  double pose7[7];       /* mTruthPosInCameraFrame.pose (tx, ty, tz, qx, qy, qz, qw): fromMinimalVector(X, Y - h / 2, Z, 0, ry, 0) */
} ps_detection;
/* what the object chain leaves per frame, sequence and detection slot */
typedef struct ps_object_stat {
  int32_t id;             /* the detection's id, -1 for an empty slot                                                          */
  int32_t n, stereo;      /* object features of the detection / of which with depth                                            */
  int32_t tracked;        /* the detection has a MapObject after the frame                                                     */
  int32_t is_new;         /* MapObjectInit ran in this frame                                                                   */
  int32_t track_ok;       /* DetectionObject::mbTrackOK at the end of TrackObjectLocalMap                                      */
  int32_t inliers;        /* mnMatchesInliers                                                                                  */
  int32_t bf_matches;     /* SearchByBruceMatching's return value                                                              */
  int32_t lm_candidates;  /* local points that passed isInFrustum                                                              */
  int32_t lm_matches;     /* SearchByProjection(F, nOrder, MOPs)'s return value                                                */
  int32_t map_points;     /* the frame's MapObjectPoints with observations when the frame was finished                         */
  int32_t reinit;         /* MapObjectReInit ran                                                                               */
  int32_t dynamic;        /* DetectionObject::GetDynamicFlag() after Tracking::DynamicStaticDiscrimination (Tracking.cc:2058)  */
  int32_t mo_dynamic;     /* its MapObject's GetDynamicFlag(), -1 without a MapObject                                          */
  int32_t dyn_n_mono, dyn_n_stereo;   /* points the two averages below were taken over (after the 5 x median rejection)        */
  double tco[7];          /* GetCFInFrameObjState(frame).pose when the frame was finished                                      */
  double dyn_mono, dyn_stereo;        /* mdMonoDynaVal / mdStereoDynaVal: mean chi2 of "the object did not move" (0: not run)  */
} ps_object_stat;
int ps_tracker_step_slot_device(ps_tracker* t, const uint8_t* d_imgs, int stride, size_t image_pitch, const uint8_t* d_masks, int mask_stride,
                                size_t mask_pitch, const ps_detection* d_dets);
/* Blocks, then copies the object results of steps [first_step, first_step + nsteps): [nsteps][n_sequences][max_objects]. */
int ps_tracker_fetch_objects(ps_tracker* t, int first_step, int nsteps, ps_object_stat* out);
int ps_tracker_sync(ps_tracker* t);
int ps_tracker_steps(const ps_tracker* t, int* steps);
/* Blocks, then copies the results of steps [first_step, first_step + nsteps): tcw [nsteps][n_sequences][16] (mTcw row-major,
 * all zero for a frame without a pose) and stats [nsteps][n_sequences]; either pointer may be NULL.  A frame whose search windows
 * overflowed the candidate store says so in its own ps_track_stat::overflowed; the call itself succeeds. */
int ps_tracker_fetch(ps_tracker* t, int first_step, int nsteps, float* tcw, ps_track_stat* stats);
/* Test hook: the next queued step reports `count` overflowed windows for sequence `seq`. */
int ps_tracker_debug_set_overflow(ps_tracker* t, int seq, int count);
/* All sequences back to NOT_INITIALIZED, step counter 0. */
int ps_tracker_reset(ps_tracker* t);
/* GPU time per stage of a step (HIP events on the tracker's stream, mean over the recorded steps, at most 64):
 * orb_extract, stereo_match, track_glue, search_by_projection, pose_optimization, and with objects: object_features,
 * object_stereo_match, object_glue, object_bruteforce, object_cfse3, object_search_by_projection. */
int ps_tracker_enable_stage_timing(ps_tracker* t, int enable);
int ps_tracker_stage_times(ps_tracker* t, const char** names, float* ms, int cap, int* n);
/* The extractor the tracker owns (its per-kernel stage times, debug reads). */
int ps_tracker_orb(ps_tracker* t, ps_orb** orb);

#ifdef __cplusplus
}
#endif
#endif /* POINTSLOT_HIP_H */
