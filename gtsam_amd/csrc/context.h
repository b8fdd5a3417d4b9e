// context.h -- device-resident state of one LM problem (one handle = one GPU = one shard).
//
// HBM layout (all FP64 unless noted; see DESIGN.md "Data layout"):
//   values / trial          packed gtsam::Values, variable-id order (12 | 17 | 3 doubles per variable)
//   *_J                     per-factor whitened records [A1 | A2 | b], AoS, written once per linearize
//   Hd, gred0               reduced variables: d x d diagonal blocks (stride 81) and gradient (stride 9)
//   V, gp                   landmarks: 3x3 blocks (stride 9) and gradient (stride 3)
//   Hoff                    off-diagonal reduced blocks from BetweenFactors (stride 81)
//   E                       per landmark-observation  E = Jc^T Jp L^-T  (stride 27), rebuilt per lambda
//   S                       reduced system BY TILES: one contiguous 128 x 128 slot per stored tile of the lower triangle
//                           (plan.slot: tile -> slot) plus the tiles of one extra tile row whose first row carries the rhs (g^T -> y^T)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <exception>
#include <memory>
#include <thread>
#include <vector>

#include "../../include/gtsam_amd.h"
#include "tile_plan.h"   // kTile, kSub; CholLists / DfLists: the host halves of the two plans below

namespace gt {

// ---- storage of the reduced system: BY TILES -----------------------------------------------------------------------------
// Every 128 x 128 tile of the lower triangle that the symbolic factorisation says can become non-zero (fill included), and every
// tile of the rhs row (tile row nt: row 0 of those tiles carries the right-hand side through the factorisation), owns one
// contiguous slot of 128 x 128 doubles, row-major with pitch 128; slot[I * nt + J] is its index, -1 for a tile that is never
// touched (what the reference keeps per clique as SymmetricBlockMatrix blocks, base/SymmetricBlockMatrix.h:195-237).  Rounds 1-3
// kept the whole (NP + 128) x NP array: 1.9 GB for the 15 507 columns of the L1723 shape with 45 % of the tiles ever touched,
// 31 GB for a 20 000-pose graph with a few per cent.
struct SMat {
  double* p; const int32_t* slot; int nt;
  __host__ __device__ __forceinline__ double* tile(int I, int J) const { return p + (int64_t)slot[(int64_t)I * nt + J] * kTileDoubles; }
  // entry (r, c) of the matrix in scalar coordinates (r = 128 nt: the rhs row)
  __host__ __device__ __forceinline__ double* at(int64_t r, int64_t c) const { return tile((int)(r >> 7), (int)(c >> 7)) + ((r & 127) << 7) + (c & 127); }
  // the same for writers of whole variable blocks: a d x d block that straddles a tile boundary next to the diagonal has entries in a
  // tile of the UPPER triangle, which has no slot (and which nobody reads): nullptr there
  __host__ __device__ __forceinline__ double* at_stored(int64_t r, int64_t c) const {
    const int32_t q = slot[(r >> 7) * nt + (c >> 7)];
    return q < 0 ? nullptr : p + (int64_t)q * kTileDoubles + ((r & 127) << 7) + (c & 127);
  }
};


// scalar slots reduced on the device (doubles)
// SC_TIMEOUT directly follows SC_FAIL: the factorisation gets `scalars + SC_FAIL` and raises [0] for a non-positive pivot, [1] for a
// dependency wait that ran into its bound (a scheduling problem, reported as an error -- never as "not positive definite")
// SC_UNSUPPORTED: a smart factor met a case in which the reference throws out of linearize() / error(): 1 = Cal3Bundler::calibrate did
// not converge, kUnsupportedCheirality = CheiralityException (a failed track's point at infinity behind one of its cameras); summed over
// the shards, so the second code lies above any count of the first
constexpr double kUnsupportedCheirality = 1024.0;
enum { SC_ERROR = 0, SC_LIN0 = 1, SC_LIN1 = 2, SC_TRIAL_ERROR = 3, SC_DELTA_SQ = 4, SC_FAIL = 5, SC_TIMEOUT = 6, SC_UNSUPPORTED = 7, SC_COUNT = 8 };

// One block of device memory, owned: released by the destructor (to the runtime, or to the process' cache of big blocks:
// device_memory.hip), movable, not copyable.  free() releases early on purpose.  Never declare one at namespace scope or as
// `static` / `thread_local`: its destructor would call the runtime during process teardown, when the runtime may be gone.
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  size_t cap = 0;                               // bytes of the allocation behind p (>= n elements: device_memory.hip keeps and re-issues big blocks)
  DevBuf() = default;
  ~DevBuf() { free(); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n), cap(o.cap) { o.p = nullptr; o.n = 0; o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { free(); p = o.p; n = o.n; cap = o.cap; o.p = nullptr; o.n = 0; o.cap = 0; }
    return *this;
  }
  void alloc(size_t count);
  void upload(const T* host, size_t count, hipStream_t s);
  void free();
};

// Tile-sparse schedule of the reduced-system Cholesky (built once per graph by the host symbolic analysis):
// which 128x128 tiles exist after fill-in, at the granularity of 256-wide column pairs.
constexpr int kEStride = 32;                    // doubles per E slot (one per observation): 9x3 block padded to 256 bytes = two 128-byte lines

struct CholPlan : CholLists {                    // + the device copies (tile_plan.h: the host half and the planner)
  DevBuf<int32_t> rows, pairs, bcols;           // concatenated lists: TRSM row tiles, SYRK (I,J) pairs, backward column tiles
  DevBuf<int32_t> bwd_col_off, bwd_col_rows;    // the backward tiles by column: offsets (nt + 1), row tiles in descending order
  DevBuf<int32_t> stored;                       // every stored tile (I,J) incl. the rhs row, in SLOT order: tile q of this list lives in slot q of S
  DevBuf<int32_t> slot;                         // (nt + 1) x nt: tile (I, J) -> its slot in S, -1 = never touched (chol_device.h::SMat); h_slot on the device
  DevBuf<int32_t> exch;                         // the stored tiles that can be non-zero BEFORE the factorisation (no fill): what a multi-GPU
                                                // exchange of the partial reduced systems has to carry (L1723: 19 % fewer than `stored`); n_exch of them
};


// Dataflow schedule of the same factorisation (chol_dataflow.hip): one task per stored 128x128 tile, left-looking, executed by
// persistent workgroups that take tasks in a fixed topological order; dependencies are epoch-stamped flags in HBM.
struct DfPlan : DfLists {                       // + the device copies (tile_plan.h: the host half and the planner)
  DevBuf<int32_t> tasks;                        // 12 per task: I, J, offset / count into klist, piece r of R (the last piece finishes the tile), slots, accumulator lanes
  DevBuf<long long> part_flag;                  // n_flag_words, by slot: kPieceBase epoch + pieces of the tile's contraction that are in
  DevBuf<int32_t> has_sub;                      // per diagonal tile J: kChainWords -- its slot, the slot of tile (J, J-1) where h_has_sub says it is stored (its update is streamed by the chain kernel) and that tile's sub-tile mask
  DevBuf<int32_t> klist;                        // contraction lists: the column tiles k < J with both (I, k) and (J, k) stored; 6 words per step: the two slots, then the
                                                // 64-bit sub-tile masks of (I, k) and (J, k) (bit 8 r + q: rows 16 r.., columns 16 q.. can be non-zero)
  DevBuf<long long> tile_flag;                  // by slot: epoch in which the tile became final
  DevBuf<long long> pd_flag;                    // by slot: epoch in which the diagonal tile received all its updates
  DevBuf<int32_t> ctrl;                         // [0] ticket counter of the bulk queue; [8..15] record of the first wait that gave up
  DevBuf<long long> trace;                      // GTG_DF_TRACE=1: 4 stamps per task + 2 per diagonal tile (gtg_debug_df_trace)
  DevBuf<int32_t> chain_off, chain_tiles;       // h_chain_off, h_chain_tiles on the device
};

// The form of the projection range: what its records look like and which kernels linearise and evaluate it.  Decided once per
// upload (upload.hip::upload_projection) from facts of the WHOLE graph -- a shard may own none of the factors that define the form.
// These six are the only states: pose-type smart factors beside stereo or bearing / range factors are refused by SmartView
// (upload.hip), bearing / range factors alone already make a three-row graph, a planar graph has no other observation, and a fisheye
// calibration is refused wherever the form would not be Rows2 without it.
enum class ProjForm {
  Rows2,        // GenericProjectionFactors only: records [A1 2x6 | A2 2x3 | b 2], two measurement entries
  Rows2Smart,   // ... and the measurements of pose-type smart factors behind them (gtg_context::smart_pose, which this state is derived from)
  Rows3,        // the graph has a GenericStereoFactor: three-row records and three measurement entries for every observation of the range
  Rows3Sam,     // the graph has bearing / range factors (with or without stereo factors): the same records, the sam factors in [n_cam, n_proj)
  Planar,       // a POSE2 / POINT2 graph: the range is its bearing / range factors alone, the POSE2 as the "camera" (reduced dimension 3):
                // records [A1 3x3 | A2 3x3 | b 3] with a zero third landmark column (the POINT2 padded to the landmark slot)
  Rows2Fisheye, // GenericProjectionFactors only, some calib row a Cal3Fisheye (FactorTables::calib_model): the records and measurement
                // entries of Rows2, so every reader of the records runs what it runs for Rows2; kernels of its own linearise and evaluate the range
};
constexpr int proj_rows(ProjForm f) { return f == ProjForm::Rows2 || f == ProjForm::Rows2Smart || f == ProjForm::Rows2Fisheye ? 2 : 3; }
constexpr int proj_dc(ProjForm f) { return f == ProjForm::Planar ? 3 : 6; }   // tangent dimension of the range's "camera"
constexpr int proj_rec(ProjForm f) { return proj_rows(f) * (proj_dc(f) + 4); }   // doubles per record [A1 R x DC | A2 R x 3 | b R]: kProjRec / kStereoRec / kPlanarRec (factors.h)
constexpr bool has_sam(ProjForm f) { return f == ProjForm::Rows3Sam; }

struct FactorTables {
  // SFM
  int64_t n_sfm = 0;
  DevBuf<int32_t> sfm_cam, sfm_point, sfm_noise;
  DevBuf<int32_t> sfm_cam_at, sfm_point_at;   // where the factor's camera / point start in the packed values (val_off of the two ids: one dependent gather less per recomputed record, fused.h)
  DevBuf<double> sfm_z, sfm_J;
  // projection
  int64_t n_proj = 0;
  DevBuf<int32_t> proj_pose, proj_point, proj_noise, proj_calib, proj_sensor;
  DevBuf<double> proj_z, proj_J, calib, sensor;
  ProjForm form = ProjForm::Rows2;
  // ProjForm::Rows2Fisheye: the camera model of every calib row (GTG_CALIB_*), a buffer of its own beside the calib table, whose
  // fisheye rows hold fx fy s u0 v0 k1 k2 k3 k4.  Empty in every other form.
  DevBuf<int32_t> calib_model;
  // GenericStereoFactor<Pose3, Point3>: the stereo factors are the observations [n_mono, n_cam) of the projection range.  A three-row
  // graph keeps three-row records (kStereoRec) and three measurement entries for every observation of the range, the monocular ones
  // with a zero third row.
  int64_t n_mono = 0;
  DevBuf<double> calib_baseline;   // [n_calib] Cal3_S2Stereo::baseline
  // BearingRangeFactor / RangeFactor / BearingFactor <Pose3, Point3> (gtsam/sam): the observations [n_cam, n_proj) of the projection
  // range, behind the stereo factors [n_mono, n_cam).  They read no calib or sensor entry (proj_calib / proj_sensor hold -1 for them) and
  // keep their measurements in an array of their own: sam_z[4 (i - n_cam)] = the measured Unit3, then the range; sam_kind GTG_SAM_*.
  // Without sam factors n_cam == n_proj and both buffers are empty.
  // ProjForm::Planar: the range is the planar bearing / range factors alone (n_mono == n_cam == 0); the two buffers hold their kinds
  // and measurements, sam_z[3 i] = (c, s) of the measured Rot2, then the range.
  int64_t n_cam = 0;
  DevBuf<int32_t> sam_kind;
  DevBuf<double> sam_z;
  // between
  int64_t n_between = 0;
  DevBuf<int32_t> between_v1, between_v2, between_noise;
  DevBuf<double> between_z, between_J;
  // prior
  int64_t n_prior = 0;
  DevBuf<int32_t> prior_var, prior_noise;
  DevBuf<int64_t> prior_off;
  DevBuf<double> prior_data, prior_J;
  // PoseTranslationPrior / PoseRotationPrior <Pose3 | Pose2> (GTG_FAC_POSE_PARTIAL): the factors [n_user_prior, n_prior) of the prior
  // range, behind the caller's PriorFactors.  Their records are prior records of the pose's tangent dimension with the rows they do not
  // have exactly 0, so every reader of prior_var / prior_J (assembly, linear error, Hessian diagonal, PCG, the incidence lists) sees more
  // priors and nothing else; prior_off / prior_data have no entry for them.  Only k_lin_pose_partial and k_error_pose_partial evaluate
  // them: partial_kind[i - n_user_prior] GTG_POSE_PARTIAL_*, partial_z[9 (i - n_user_prior)] the measurement.  Without such factors
  // n_user_prior == n_prior and both buffers are empty.
  int64_t n_user_prior = 0;
  DevBuf<int32_t> partial_kind;
  DevBuf<double> partial_z;
};

}  // namespace gt

namespace gt {
// Streams and events of the factorisation schedule (cholesky.hip) -- owned by the handle: streams and events belong to
// the device they were created on, and two handles driven from two host threads must not share them.
struct CholStreams {
  hipStream_t panel = nullptr;    // high-priority stream of the serial panel chain (the bulk updates run on the handle's stream)
  hipEvent_t start = nullptr;
  std::vector<hipEvent_t> P, N;   // per column pair: rest(p) finished / chain of pair p finished
  CholStreams() = default;
  CholStreams(const CholStreams&) = delete;
  CholStreams& operator=(const CholStreams&) = delete;
  ~CholStreams() {
    if (panel) (void)hipStreamDestroy(panel);
    if (start) (void)hipEventDestroy(start);
    for (auto* v : {&P, &N}) for (hipEvent_t e : *v) (void)hipEventDestroy(e);
  }
};
struct HostIndex;   // analysis.h: host copy of the factor index arrays the symbolic analysis reads
}  // namespace gt

// Everything a handle owns is released by its destructor; gtg_destroy (api.hip) decides WHEN and on which device that runs.
struct gtg_context {
  gtg_context();
  ~gtg_context();   // joins block_level_thread first (its closure writes into this object); both in device_memory.hip, where HostIndex is complete
  int device = 0;
  hipStream_t stream = nullptr;
  gt::CholStreams cs;
  std::vector<hipEvent_t> phase_events;   // 2 per phase (gtg_enable_timing)
  hipStream_t copy_stream = nullptr;      // non-blocking: the uploads that run beside the symbolic analysis (gtg_upload_problem)
  int shard = 0, n_shards = 1;
  bool uploaded = false, linearized = false, have_trial = false;

  // ---- variables -------------------------------------------------------------------------------
  int32_t n_vars = 0;
  std::vector<int32_t> h_var_type;
  std::vector<int64_t> h_val_off, h_dim_off;   // size n_vars+1
  int64_t val_size = 0, dim_size = 0;
  // Smart factors (SmartProjectionFactor): every factor owns a HIDDEN landmark variable (ids n_user_vars .. n_vars-1, appended
  // behind the caller's variables, so the caller's values / tangent vectors are prefixes of the device's) that is re-triangulated
  // from the cameras instead of being optimised; its measurements are GeneralSFM observations smart_obs0 .. of the sfm tables
  // (camera-type factors; pose-type factors: smart_pose below).
  int32_t n_user_vars = 0;
  int64_t user_val_size = 0, user_dim_size = 0;
  int64_t n_smart = 0, smart_obs0 = 0;
  gt::DevBuf<int64_t> smart_ptr;            // [n_smart + 1] measurements of a factor, relative to smart_obs0
  gt::DevBuf<double> smart_params;          // 8 per factor (include/gtsam_amd.h)
  // per factor: 0 VALID, 1 DEGENERATE, 2 BEHIND_CAMERA, 3 OUTLIER, 4 FAR_POINT (triangulation.h:611-612), + 16 (kTriAtInfinity) when this
  // use of a failed track replaces the landmark by a point at infinity.  TWO arrays: smart_lin_status is
  // the outcome at the LINEARISATION point (written by gtg_linearize only; read by everything that builds the linear system, which
  // stays fixed over the lambda retries of an iteration as the reference's linearised Hessian factor does); smart_status the
  // outcome of the most recent ERROR evaluation (gtg_error, the trial point of a lambda try), read by k_error only
  gt::DevBuf<int32_t> smart_status, smart_lin_status;
  gt::DevBuf<int32_t> smart_cache_state;    // per factor: -1 nothing cached, else the cached status
  gt::DevBuf<double> smart_cache_pose;      // 12 per measurement: the camera poses of the cached triangulation
  gt::DevBuf<double> smart_cache_point;     // 3 per factor
  // TriangulationParameters::useLOST (smart_params[8 i + 7] > 0 on some factor of the WHOLE graph): the LOST form of the triangulation
  // kernel is launched, and smart_lost_rows holds its work space -- 8 doubles per smart measurement of this shard.  Empty otherwise.
  bool smart_lost = false;
  gt::DevBuf<double> smart_lost_rows;
  const int32_t* smart_last_status = nullptr;   // smart_status or smart_lin_status: what the last gtg_error / gtg_linearize wrote (gtg_get_smart_triangulation)
  // SmartProjectionPoseFactor<Cal3_S2> (gtg_problem.smart_calib >= 0): the measurements are PROJECTION observations smart_obs0 .. of
  // the proj tables instead (keys POSE3, one shared Cal3_S2, optional body_P_sensor); a graph has smart factors of one kind only.  f.form is ProjForm::Rows2Smart exactly when this is set
  bool smart_pose = false;
  // SmartProjectionRigFactor (gtg_problem.smart_calib == GTG_SMART_RIG) joins the same range with a calib / sensor entry per measurement
  // and may name a pose several times in one track.  smart_repeats: some rig-type track of the WHOLE graph does; then rep_* list this
  // shard's sightings of such (pose, track) groups, CSR by pose variable (rep_var ascending) -> group -> observation of the projection
  // range (in range order), for the kernels that add the cross terms of a group to the Hessian diagonal and the block-Jacobi blocks
  bool smart_repeats = false;
  int32_t n_rep_vars = 0;
  gt::DevBuf<int32_t> rep_var, rep_grp_ptr, rep_obs_ptr, rep_smart, rep_obs;
  gt::DevBuf<int32_t> obs_smart, lm_smart;  // per observation of the range the smart measurements live in (GeneralSFM, or projection when smart_pose) / per landmark: its smart factor or -1
  gt::DevBuf<int32_t> var_type;
  gt::DevBuf<int64_t> val_off, dim_off;
  gt::DevBuf<double> values, trial, delta;

  // classification: landmark (POINT3 eliminated first) or reduced variable
  int32_t n_lm = 0, n_red_vars = 0;
  int64_t n_red = 0;                            // scalar dimension of the reduced system
  uint64_t structure_hash = 0;                  // identity of the layout below (ordering, offsets, padding, tile structure): equal on every shard of a job
  int32_t NP = 0;                               // padded dimension of S: n_red + alignment gaps (parts start on 256-column boundaries), multiple of kTile
  std::vector<int64_t> h_pad_index;             // the padded (identity) rows/columns of S
  gt::DevBuf<int64_t> pad_index;
  std::vector<int32_t> h_lm_index, h_red_index; // per variable: index among landmarks / reduced (or -1)
  std::vector<int32_t> h_lm_var, h_red_var;     // inverse maps
  std::vector<int32_t> h_red_pos;               // reduced index -> position in the ordering
  std::vector<int64_t> h_red_off;               // per reduced index: scalar offset in S
  std::vector<int32_t> h_red_dim;
  gt::DevBuf<int32_t> lm_var, red_var, red_dim, lm_index, red_index, lm_owned;
  gt::DevBuf<int64_t> red_off;

  // ---- noise table (inverse sigmas precomputed like the reference constructors) ------------------
  gt::DevBuf<int32_t> noise_kind, noise_rkind;
  gt::DevBuf<double> noise_rk;
  gt::DevBuf<int64_t> noise_off;
  gt::DevBuf<double> noise_data;

  gt::FactorTables f;

  // ---- incidence (host-built CSR, device copies) ---------------------------------------------------
  // observations: obs id o < n_sfm -> sfm factor o; else projection factor o - n_sfm
  int64_t n_obs = 0;
  gt::DevBuf<int32_t> obs_red, obs_lm;          // reduced index / landmark index of each observation
  gt::DevBuf<int64_t> lm_obs_ptr;  gt::DevBuf<int32_t> lm_obs;      // landmark -> observations
  gt::DevBuf<int64_t> lm_pri_ptr;  gt::DevBuf<int32_t> lm_pri;      // landmark -> prior factors
  gt::DevBuf<int64_t> red_inc_ptr; gt::DevBuf<int32_t> red_inc_kind, red_inc_idx;  // reduced var -> contributions
  int64_t n_hoff = 0;                                                // off-diagonal blocks from between factors
  gt::DevBuf<int32_t> hoff_row, hoff_col;                            // reduced indices (row pos > col pos)
  gt::DevBuf<int64_t> hoff_ptr;  gt::DevBuf<int32_t> hoff_fac;       // block -> between factors (sign bit = transposed)
  int64_t n_pairs = 0, n_pair_terms = 0;                             // Schur block pairs
  bool device_terms = false;                                         // their term lists were built on the device (device_analysis.hip)
  gt::DevBuf<int32_t> pair_row, pair_col;
  gt::DevBuf<int64_t> pair_ptr;  gt::DevBuf<int32_t> pair_oa, pair_ob;

  // ---- numeric buffers ---------------------------------------------------------------------------
  gt::DevBuf<double> Hd, gred0, hdiag_red;      // reduced diag blocks (81), gradient (9), diagonal (n_red)
  gt::DevBuf<double> V, gp;                     // landmark blocks (9) and gradient (3)
  gt::DevBuf<double> Hoff;                      // (81 per block)
  gt::DevBuf<double> Linv, ylm, E, delta_lm;    // per try: landmark L^-1 (9), y (3), E (32/obs), delta (3)
  gt::DevBuf<double> pcg_vec, pcg_bj, pcg_y;    // PCG solver: r, p, q1, q2, b (5 x NP); block-Jacobi factors (81 / reduced variable); y_l (3 / landmark)
  bool fused_sfm = false;                       // the GeneralSFM records are recomputed where they are needed instead of stored (fused.h): graphs without smart factors
  gt::DevBuf<double> wobs;                      // per try: E_o y_l (9 doubles) per entry of the cameras' contribution lists: the summands of the reduced right-hand side
  gt::DevBuf<int32_t> obs_wpos;                 // observation -> its entry in red_inc_* (where k_obs_E stores its summand)
  gt::DevBuf<double> cam_part;                  // k_cam_fused with several workgroups per camera: their partial sums
  gt::DevBuf<double> cam_pack;                  // fused.h::CamPack per entry of the camera-sorted contribution lists (4 doubles each), once per graph
  gt::DevBuf<double> vobs;                      // per try: Jp^T (Jc x_cam) of every observation (3), for the back-substitution
  gt::DevBuf<double> S;                         // plan.n_stored slots of 128 x 128 doubles: the stored tiles of the reduced system + the rhs row's tiles
  gt::DevBuf<double> yred;                      // NP: y = L^-1 g gathered from the rhs tiles for the backward solve
  gt::DevBuf<double> Dinv;                      // per diagonal tile (128x128 doubles): the four 32x32 diagonal inverses, the MFMA operand
                                                // images of the tile's sub-blocks for the TRSM, and the tile's progress word (zeroed at allocation)
  gt::DevBuf<unsigned char> pivot_kind;         // per scalar column of S: 1 / 2 = last pivot of a variable (dim >= 2 / dim 1): the rank test of
  gt::DevBuf<double> tile_exp;                  // base/cholesky.cpp:144-157 applies there; tile_exp: exponent of every tile's last pivot (carry)
  gt::DevBuf<long long> chol_epoch_dev;         // factorisations launched so far (base of the progress words): a device copy of chol_epoch (debug)
  long long chol_epoch = 0;                     // counted on the host, passed to the kernels by value
  gt::CholPlan plan;
  gt::DfPlan df;                                // the dataflow schedule (default); `plan` keeps the lists for zeroing / exchange / backward solve
  bool use_df = true;
  int64_t df_fallbacks = 0;                    // lambda tries repeated with the stream schedule after a time-out of the dataflow pass
  gt::DevBuf<double> xbuf;                      // multi-GPU: the exchanged part of S packed contiguously for the all-reduce
  // multi-GPU exchange at block granularity: every structurally non-zero d x d block of the reduced system (diagonal blocks +
  // the off-diagonal blocks of the WHOLE graph, identical on every shard), 81 doubles per block, then the rhs row and the
  // padding diagonal.  3x less than whole 128x128 tiles on the L1723 shape (0.13 GB against 0.38 GB).
  int64_t n_xb = 0;
  gt::DevBuf<int64_t> xb_row_off, xb_col_off;   // scalar offsets of the block in S (row >= col)
  gt::DevBuf<int32_t> xb_dim;                   // rows | cols << 8
  gt::DevBuf<double> xred;                      // NP solution of the reduced system
  gt::DevBuf<double> partials;                  // block partial sums for reductions
  gt::DevBuf<double> scalars;                   // SC_COUNT
  double h_scalars[gt::SC_COUNT] = {0};

  // ---- multi-GPU exchange --------------------------------------------------------------------------
  gt::DevBuf<double> layout_probe;              // 4 doubles: pieces of structure_hash summed across the shards (verify_layout)
  bool layout_verified = false;
  gtg_allreduce_fn allreduce = nullptr;
  void* allreduce_user = nullptr;

  // ---- timing ----------------------------------------------------------------------------------------
  bool timing = false;
  double phase_ms[GTG_PH_COUNT] = {0};
  int64_t phase_calls[GTG_PH_COUNT] = {0};
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  double chol_flops = 0, chol_flops_block = 0, lin_bytes = 0;
  std::thread block_level_thread;               // computes chol_flops_block beside / after analyze() (analysis.hip::join_block_level)
  std::exception_ptr block_level_err;
  std::unique_ptr<gt::HostIndex> index;         // created on first use (analysis.hip::host_index)
};

namespace gt {
inline SMat smat(const gtg_context& c) { return SMat{c.S.p, c.plan.slot.p, c.plan.nt}; }   // the handle's reduced system (context.h::SMat)
}  // namespace gt
