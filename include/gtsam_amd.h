/* gtsam_amd.h -- C ABI of the MI355X-native Levenberg-Marquardt inner loop.
 *
 * This is the drop-in boundary for ONE path of borglab/gtsam: the
 * linearize -> damp -> eliminate -> solve -> retract -> error loop of
 * gtsam::LevenbergMarquardtOptimizer.  GTSAM has no FFI/plugin ABI of its own; its extension
 * point is C++ subclassing (NonlinearOptimizer::iterate() nonlinear/NonlinearOptimizer.h:136,
 * LevenbergMarquardtOptimizer::linearize() LevenbergMarquardtOptimizer.h:112-113,
 * NonlinearOptimizer::solve() NonlinearOptimizer.h:129-130).  The functions below are what a
 * subclass overriding iterate() binds to (see INTEGRATION.md for the GTSAM-side shim and
 * gtsam_amd/host/ for the shipped one).  Each entry point cites the reference code it replaces.
 *
 * Conventions: extern "C"; plain pointers + explicit sizes; all host arrays are caller-owned and
 * copied during the call; int status returns (GTG_OK=0, GTG_INDETERMINATE=1 means "the damped
 * system was not positive definite" = where the reference throws
 * IndeterminantLinearSystemException, linear/HessianFactor.cpp:476-483, and LM raises lambda,
 * nonlinear/LevenbergMarquardtOptimizer.cpp:154-160; negative = usage / HIP error, message via
 * gtg_last_error()).  No exceptions cross the boundary, no GTSAM or torch types appear.
 * All floating point is IEEE double (gtsam::Matrix = Eigen::MatrixXd, base/Matrix.h:39).
 */
#ifndef GTSAM_AMD_H
#define GTSAM_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gtg_context* gtg_handle;

enum { GTG_OK = 0, GTG_INDETERMINATE = 1, GTG_ERR_USAGE = -1, GTG_ERR_HIP = -2,
       GTG_ERR_UNSUPPORTED = -3 };

/* Variable (gtsam::Value) types and their packed storage.
 *   POSE3      gtsam::Pose3 (geometry/Pose3.h): 12 doubles = R row-major (9) then t (3); tangent 6 = [omega; v]
 *   SFM_CAMERA gtsam::PinholeCamera<Cal3Bundler> (geometry/PinholeCamera.h, Cal3Bundler.h):
 *              17 doubles = pose (12) then f,k1,k2,u0,v0; tangent 9 = [pose(6); f,k1,k2]
 *   POINT3     gtsam::Point3: 3 doubles; tangent 3
 *   POSE2      gtsam::Pose2 (geometry/Pose2.h): 3 doubles = x, y, theta (theta() = atan2(s, c), wrapped); tangent 3,
 *              retract = compose with Pose2(v0, v1, v2) (Pose2.cpp:99-109, GTSAM_SLOW_BUT_CORRECT_EXPMAP off)
 *   POINT2     gtsam::Point2, the landmark of a planar graph, padded to the POINT3 slot: 3 doubles = x, y, 0; tangent 3 =
 *              dx, dy, 0.  Given a third storage entry of 0, every third entry the library returns (delta, gradients, Hessian
 *              diagonal, trial and accepted values) is exactly 0.0.  Only in a graph of POSE2 / POINT2 variables.             */
enum { GTG_VAR_POSE3 = 0, GTG_VAR_SFM_CAMERA = 1, GTG_VAR_POINT3 = 2, GTG_VAR_POSE2 = 3, GTG_VAR_POINT2 = 4 };

/* Factor types on the path. */
enum { GTG_FAC_GENERAL_SFM = 0,   /* GeneralSFMFactor<PinholeCamera<Cal3Bundler>,Point3>  slam/GeneralSFMFactor.h:127-177 */
       GTG_FAC_PROJECTION = 1,    /* GenericProjectionFactor<Pose3,Point3,Cal3_S2>        slam/ProjectionFactor.h:138-166 */
       GTG_FAC_BETWEEN_POSE3 = 2, /* BetweenFactor<Pose3>, or BetweenFactor<Pose2> when its  slam/BetweenFactor.h:111-124
                                     two variables are POSE2 (same table, see between_z)                                  */
       GTG_FAC_PRIOR = 3,         /* PriorFactor<T>                                        nonlinear/PriorFactor.h:98-102 */
       GTG_FAC_STEREO = 4,       /* GenericStereoFactor<Pose3,Point3>                     slam/StereoFactor.h:126-154:
                                     residual h(x) - z with THREE rows (uL, uR, v), h = StereoCamera::project2
                                     (geometry/StereoCamera.cpp:37-79) with a Cal3_S2Stereo (fx, fy, u0, v0 and a baseline; the skew is
                                     stored and not used, as there); body_P_sensor: H1 = H1 * H0 of pose.compose(sensor, H0) (:129-135);
                                     q.z <= 0 (StereoCheiralityException, throwCheirality_ = false): both Jacobians zero, residual
                                     Vector3::Constant(2 fx) (:144-153).  Its landmark is eliminated like a projection factor's. */
       GTG_FAC_SAM = 5 };         /* BearingRangeFactor / RangeFactor / BearingFactor <Pose3,Point3>   sam/BearingRangeFactor.h,
                                     sam/RangeFactor.h, sam/BearingFactor.h (ExpressionFactorN, nonlinear/ExpressionFactor.h:104-153):
                                     h = Pose3::bearing / Pose3::range of the landmark (geometry/Pose3.cpp:399-439), b = Local(h, z)
                                     (BearingRange.h:138-144, Unit3::localCoordinates geometry/Unit3.cpp:285-303, in the basis of the
                                     PREDICTED direction), Jacobians those of h alone, the whole system whitened (:147-150).  Rows:
                                     bearing-range 3 (bearing 0-1, range 2), range 1, bearing 2.  Its landmark is eliminated like a
                                     projection factor's. */
/* sam_kind */
enum { GTG_SAM_BEARING_RANGE = 0, GTG_SAM_RANGE = 1, GTG_SAM_BEARING = 2 };

/* Noise models (linear/NoiseModel.cpp).  whiten(v) is
 *   UNIT v ; ISOTROPIC v*invsigma (:641-663) ; DIAGONAL v.*invsigmas (:311-325) ; GAUSSIAN R*v (:163-181)
 * noise_data holds the constructor arguments: UNIT nothing; ISOTROPIC {sigma}; DIAGONAL sigmas[dim];
 * GAUSSIAN R[dim*dim] row-major (upper-triangular sqrt information).  The library derives
 * invsigma = 1.0/sigma exactly like the reference constructors do (NoiseModel.cpp:275-281). */
enum { GTG_NOISE_UNIT = 0, GTG_NOISE_ISOTROPIC = 1, GTG_NOISE_DIAGONAL = 2, GTG_NOISE_GAUSSIAN = 3 };

/* Optional m-estimator wrapped around a noise-table entry = noiseModel::Robust(robust, noise)
 * (linear/NoiseModel.h:678-740, linear/LossFunctions.cpp), Block re-weighting scheme (the default):
 * whitened system scaled by sqrt(weight(||whitened b||)) (LossFunctions.cpp:51-124), factor error =
 * loss(||whitened r||) (NoiseModel.h:716-718).  Parameter = the estimator's modelParameter() (c or k).
 * As in the reference, GTG_FAC_GENERAL_SFM factors are NOT re-weighted when they linearize (their own linearize()
 * whitens H1, H2, b one at a time through Robust::Whiten(Matrix), slam/GeneralSFMFactor.h:162-168, where the
 * weight evaluates to 1); the m-estimator only enters their error(). */
enum { GTG_ROBUST_NONE = 0, GTG_ROBUST_FAIR = 1, GTG_ROBUST_HUBER = 2, GTG_ROBUST_CAUCHY = 3, GTG_ROBUST_TUKEY = 4,
       GTG_ROBUST_WELSCH = 5, GTG_ROBUST_GEMANMCCLURE = 6, GTG_ROBUST_DCS = 7, GTG_ROBUST_L2WITHDEADZONE = 8 };
/* (AsymmetricTukey / AsymmetricCauchy, LossFunctions.cpp:433-500: on this path the distance is a norm, >= 0, where they coincide with
 * Tukey / Cauchy -- the C++ shim maps them.) */

/* The factor graph in structure-of-arrays form: what the extractor produces by walking a
 * gtsam::NonlinearFactorGraph once (FactorGraph.h:92 factors_, Factor.h keys_). Variable ids are
 * dense 0..n_vars-1 (the shim maps gtsam::Key -> id in Values order, Values.h:74-79). */
/* GTG_FAC_SAM2: BearingRangeFactor<Pose2, Point2>, RangeFactor<Pose2, Point2> and BearingFactor<Pose2, Point2> (gtsam/sam), the
 * landmark factors of planar SLAM.  The same ExpressionFactorN as GTG_FAC_SAM with h = Pose2::bearing (geometry/Pose2.cpp:245-256:
 * Rot2::relativeBearing of transformTo, a ZERO Jacobian and the identity rotation at a distance <= 1e-5) and Pose2::range
 * (Pose2.cpp:270-284: norm2, Jacobian (1, 1) at r <= 1e-10); b = [theta(h^-1 z) ; z_range - h_range].  Rows: bearing-range 2
 * (bearing 0, range 1), range 1, bearing 1.  A POINT2 is a landmark and is eliminated like a POINT3; a graph with a POINT2 variable is
 * a PLANAR graph: beside these factors it may hold BetweenFactor<Pose2>, PriorFactor<Pose2> and the 2-D partial pose priors.
 * NULL / 0: no such factors.  Refused by gtg_upload_problem, each with its own message: keys that are not (POSE2, POINT2); an unknown
 * kind; a noise dimension that does not match the kind (2, 1, 1); n_sam2 > 0 with a table missing; a POINT2 variable or a planar
 * factor in a graph that also has POSE3, SFM_CAMERA or POINT3 variables or camera, stereo, 3-D bearing / range or smart factors; a
 * PriorFactor on a POINT2; n_shards > 1.  gtg_try_lambda_pcg refuses a planar graph at the call.
 * The table is a struct of its own, held by value as `planar`, the LAST member of gtg_problem: in memory its six fields stand where six
 * more fields of gtg_problem would, behind the partial pose priors, and gtg_problem's own field list is what it was (a caller built
 * against the older struct must be recompiled all the same). */
typedef struct gtg_planar_table {
  int64_t n_sam2;
  const int32_t* sam2_kind;       /* [n_sam2] GTG_SAM_* */
  const int32_t* sam2_pose;       /* [n_sam2] variable id of the POSE2 */
  const int32_t* sam2_point;      /* [n_sam2] variable id of the POINT2 */
  const double* sam2_z;           /* [n_sam2*3] c_z, s_z of the measured Rot2 as the reference holds it, then the measured range; the
                                     entries a kind does not use are 0 */
  const int32_t* sam2_noise;      /* [n_sam2] index into the noise table (dim 2, 1 or 1 by kind) */
} gtg_planar_table;

typedef struct gtg_problem {
  int32_t n_vars;
  const int32_t* var_type;       /* [n_vars] GTG_VAR_* */

  int32_t n_noise;               /* shared noise-model table */
  const int32_t* noise_kind;     /* [n_noise] GTG_NOISE_* */
  const int32_t* noise_dim;      /* [n_noise] */
  const int64_t* noise_off;      /* [n_noise] offset into noise_data */
  const double* noise_data;
  const int32_t* noise_robust;   /* [n_noise] GTG_ROBUST_* or NULL (no robust models) */
  const double* noise_robust_param; /* [n_noise] c / k of the m-estimator */

  int64_t n_sfm;                 /* GTG_FAC_GENERAL_SFM */
  const int32_t* sfm_cam;        /* [n_sfm] variable id of the SFM_CAMERA */
  const int32_t* sfm_point;      /* [n_sfm] variable id of the POINT3 */
  const double* sfm_z;           /* [n_sfm*2] measured pixel */
  const int32_t* sfm_noise;      /* [n_sfm] index into noise table (dim 2) */

  int64_t n_proj;                /* GTG_FAC_PROJECTION */
  const int32_t* proj_pose;      /* [n_proj] variable id of the POSE3 */
  const int32_t* proj_point;     /* [n_proj] variable id of the POINT3 */
  const double* proj_z;          /* [n_proj*2] */
  const int32_t* proj_noise;     /* [n_proj] */
  const int32_t* proj_calib;     /* [n_proj] index into calib table */
  const int32_t* proj_sensor;    /* [n_proj] index into sensor table or -1 (body_P_sensor_ absent) */
  int32_t n_calib;
  const double* calib;           /* [n_calib*5] Cal3_S2 fx,fy,s,u0,v0 (geometry/Cal3_S2.cpp:44-50); distortion: calib_distortion below */
  int32_t n_sensor;
  const double* sensor;          /* [n_sensor*12] body_P_sensor poses */

  int64_t n_between;             /* GTG_FAC_BETWEEN_POSE3 */
  const int32_t* between_v1;     /* [n_between] */
  const int32_t* between_v2;     /* [n_between] */
  const double* between_z;       /* [n_between*12] measured relative pose (Pose3 packing; for a POSE2 pair x, y, theta
                                    in the first 3 doubles of the factor's 12) */
  const int32_t* between_noise;  /* [n_between] (dim 6, or 3 for a POSE2 pair) */

  int64_t n_prior;               /* GTG_FAC_PRIOR */
  const int32_t* prior_var;      /* [n_prior] */
  const int64_t* prior_off;      /* [n_prior] offset into prior_data (storage size of the var type) */
  const double* prior_data;
  const int32_t* prior_noise;    /* [n_prior] (dim = tangent dim of the variable) */

  const double* calib_distortion; /* [n_calib*4] k1, k2, p1, p2 of a Cal3DS2 calibration (radial + tangential distortion,
                                     geometry/Cal3DS2_Base.cpp:93-132: GenericProjectionFactor<Pose3, Point3, Cal3DS2>), or NULL:
                                     every entry of the calib table is a plain Cal3_S2.  (Appended in round 2: a caller built
                                     against the older struct must be recompiled.) */

  /* SmartProjectionFactor<PinholeCamera<Cal3Bundler>> (slam/SmartProjectionFactor.h, the factor of timing/timeSFMBALsmart.cpp), or --
   * with smart_calib at the end of this struct -- SmartProjectionPoseFactor<Cal3_S2> or SmartProjectionRigFactor<PinholePose<Cal3_S2>>:
   * one factor = one track; its landmark is NOT a variable but re-triangulated from the cameras at every linearisation / error
   * evaluation (DLT, geometry/triangulation.cpp:27-57, checks of triangulateSafe triangulation.h:697-752, cached while no camera
   * pose moves by more than retriangulationThreshold, SmartProjectionFactor.h:127-183) and eliminated without damping (the Schur
   * complement of the point, :190-233; JacobianFactorQ / JacobianFactorSVD are the same normal equations).  NULL / 0: no smart factors. */
  int64_t n_smart;
  const int64_t* smart_ptr;       /* [n_smart+1] offsets of a factor's measurements in smart_cam / smart_z (>= 1 measurement each) */
  const int32_t* smart_cam;       /* variable id (SFM_CAMERA; POSE3 for a pose-type or rig-type factor, where a rig-type factor may
                                     name a pose several times) of every measurement */
  const double* smart_z;          /* 2 per measurement */
  const int32_t* smart_noise;     /* [n_smart] index into the noise table (dim 2, Unit or Isotropic as the reference requires) */
  const double* smart_params;     /* [n_smart*8] rankTolerance, landmarkDistanceThreshold, dynamicOutlierRejectionThreshold,
                                     retriangulationThreshold, degeneracyMode (0 IGNORE_DEGENERACY, 1 ZERO_ON_DEGENERACY,
                                     2 HANDLE_INFINITY), linearizationMode (0 HESSIAN, 2 JACOBIAN_Q, 3 JACOBIAN_SVD; 1 =
                                     IMPLICIT_SCHUR is refused: the reference's direct solvers cannot eliminate it either),
                                     enableEPI (0 / 1: the DLT point refined by the reference's LM on TriangulationFactors,
                                     triangulation.h:211-221, 531-534), useLOST (0: DLT; > 0: triangulateLOST, geometry/triangulation.cpp:86-147,
                                     and the value is its measurement sigma -- the mean of the triangulation noise model's sigmas, or
                                     1e-4 without one, triangulation.h:503; negative or non-finite: refused.  The rank test of LOST
                                     is RELATIVE to the largest pivot of the reference's column-pivoted QR: with rankTolerance 1.0
                                     every LOST track is DEGENERATE, as in the reference).  A track that does not triangulate is what SmartProjectionFactor.h makes of it:
                                     nothing (ZERO_ON_DEGENERACY; the Jacobian modes when linearising), a point at infinity
                                     (:356-371 when linearising in HESSIAN mode, :419-427 in the error under HANDLE_INFINITY), error
                                     0.0 otherwise.  Where the reference THROWS out of
                                     linearize() / error() -- the point at infinity behind one of the track's cameras
                                     or the enableEPI refinement linearising behind a camera (CheiralityException),
                                     Cal3Bundler::calibrate not converging -- the call returns an error */

  /* GTG_FAC_STEREO: GenericStereoFactor<Pose3, Point3> (slam/StereoFactor.h), the factor of examples/StereoVOExample*.cpp.  NULL / 0: no
   * stereo factors.  (Appended after the smart tables: a caller built against the older struct must be recompiled.) */
  int64_t n_stereo;
  const int32_t* stereo_pose;     /* [n_stereo] variable id of the POSE3 */
  const int32_t* stereo_point;    /* [n_stereo] variable id of the POINT3 */
  const double* stereo_z;         /* [n_stereo*3] measured StereoPoint2: uL, uR, v */
  const int32_t* stereo_noise;    /* [n_stereo] index into the noise table (dim 3) */
  const int32_t* stereo_calib;    /* [n_stereo] index into the calib table above (fx, fy, s, u0, v0 of the Cal3_S2Stereo) */
  const int32_t* stereo_sensor;   /* [n_stereo] index into the sensor table or -1; NULL: no factor has a body_P_sensor */
  const double* calib_baseline;   /* [n_calib] Cal3_S2Stereo::baseline(); read only for the entries a stereo factor refers to; must be
                                     non-NULL when n_stereo > 0 */

  /* SmartProjectionPoseFactor<Cal3_S2> (slam/SmartProjectionPoseFactor.h, wrapped as SmartProjectionPose3Factor; the factor of
   * examples/SFMExample_SmartFactor.cpp and ISAM2Example_SmartFactor.cpp): a smart factor whose keys are POSE3 variables, with one shared
   * fixed Cal3_S2 and an optional body_P_sensor; its cameras are PinholePose<Cal3_S2>(pose * body_P_sensor, K) (:138-147), the camera
   * dimension is 6.  Such a factor uses the smart tables above -- smart_cam then holds POSE3 variable ids -- and says so here.
   * Refused by gtg_upload_problem (out of scope, not computed as something else): camera-type and pose-type smart factors in one
   * graph; pose-type smart factors beside GenericStereoFactors; a calib entry with Cal3DS2 distortion; enableEPI on a pose-type factor.
   * (Appended after the stereo tables: a caller built against the older struct must be recompiled.) */
  const int32_t* smart_calib;     /* [n_smart] index into the calib table, -1 for a camera-type smart factor, or GTG_SMART_RIG (-2,
                                     the tables at the end of this struct) for a rig-type one; NULL: all -1 */
  const int32_t* smart_sensor;    /* [n_smart] index into the sensor table or -1 (no body_P_sensor); NULL: none */

  /* GTG_FAC_SAM: BearingRangeFactor<Pose3, Point3>, RangeFactor<Pose3, Point3> and BearingFactor<Pose3, Point3> (gtsam/sam), the
   * landmark factors of a lidar, sonar, radar or UWB front end.  They use no calib or sensor entry: n_calib may be 0.  NULL / 0: no
   * such factors.  Refused by gtg_upload_problem: keys that are not (POSE3, POINT3); a noise dimension that does not match the kind
   * (3, 1, 2); an unknown kind; pose-type smart factors in the same graph (three-row records).
   * (Appended after the pose-type smart tables: a caller built against the older struct must be recompiled.) */
  int64_t n_sam;
  const int32_t* sam_kind;        /* [n_sam] GTG_SAM_* */
  const int32_t* sam_pose;        /* [n_sam] variable id of the POSE3 */
  const int32_t* sam_point;       /* [n_sam] variable id of the POINT3 */
  const double* sam_z;            /* [n_sam*4] the measured Unit3's three stored doubles (a unit vector, as the reference holds it),
                                     then the measured range; the entries a kind does not use are 0 */
  const int32_t* sam_noise;       /* [n_sam] index into the noise table (dim 3, 1 or 2 by kind) */

  /* SmartProjectionRigFactor<PinholePose<Cal3_S2>> (slam/SmartProjectionRigFactor.h: stereo, surround and multi-camera front ends): a
   * smart factor whose keys are the BODY poses and whose measurements each look through one camera of a fixed rig.  Factor i is
   * rig-type when smart_calib[i] == GTG_SMART_RIG: measurement k (an index into smart_cam / smart_z) then uses calib row
   * smart_meas_calib[k] and sensor row smart_meas_sensor[k] (-1: no extrinsic), its camera is PinholePose<Cal3_S2>(pose * body_P_sensor,
   * K) (:209-222).  smart_cam holds the NON-unique POSE3 ids in measurement order: the same pose may occur several times in one track
   * (two cameras of the rig seeing the landmark from one body pose), and the factor's Hessian is the reference's, on the unique keys
   * (:312-322).  The entries of both tables at the measurements of other factors are not read.  Both NULL and no GTG_SMART_RIG entry:
   * no rig-type factors.  Rig-type and pose-type factors may share a graph.
   * Refused by gtg_upload_problem: smart_params other than degeneracyMode 1 (ZERO_ON_DEGENERACY) and linearizationMode 0 (HESSIAN) on a
   * rig-type factor (the reference's constructor throws, :100-107); enableEPI on it; a named calib row with Cal3DS2 distortion;
   * smart_sensor[i] != -1 on it; a GTG_SMART_RIG entry with either table NULL; indices out of range; keys that are not POSE3; and what is
   * refused for pose-type factors (camera-type factors, stereo or bearing / range factors in the same graph).
   * (Appended after the bearing / range tables: a caller built against the older struct must be recompiled.) */
  const int32_t* smart_meas_calib;   /* [smart_ptr[n_smart]] index into the calib table, read for the measurements of rig-type factors */
  const int32_t* smart_meas_sensor;  /* [smart_ptr[n_smart]] index into the sensor table or -1, read for the same measurements */

  /* GTG_FAC_POSE_PARTIAL: PoseTranslationPrior<POSE> and PoseRotationPrior<POSE> (slam/PoseTranslationPrior.h, slam/PoseRotationPrior.h;
   * wrapped as PoseTranslationPrior3D / 2D and PoseRotationPrior3D / 2D), the absolute fix of PART of a pose: a position from GPS, UWB or a
   * total station, an attitude from a compass or a gravity-aligned IMU.  Unary on a POSE3 or POSE2 variable; the kind and the variable's
   * type decide the form (r the residual, H its Jacobian on the pose's tangent; b = -r, the whole system whitened, a Robust model
   * re-weights by sqrt(weight(|whitened b|))):
   *   TRANSLATION on POSE3  3 rows  r = t - z                      H = [0 | R]           z[0..2] the measured Point3
   *   ROTATION    on POSE3  3 rows  r = Logmap(Z^T R)              H = [I | 0] exactly   z[0..8] the measured Rot3, row-major
   *                                 (Rot3::localCoordinates, SO3::Logmap with its three branches; H is the identity block the
   *                                 reference writes, not the derivative of Logmap)
   *   TRANSLATION on POSE2  2 rows  r = t - z                      H = [c -s 0; s c 0]   z[0..1] the measured Point2
   *   ROTATION    on POSE2  1 row   r = theta of Rot2(c_z, -s_z) * Rot2(c, s)  H = [0 0 1]  z[0..1] = c_z, s_z as the reference's
   *                                 (Rot2::localCoordinates: wrapped into (-pi, pi])        Rot2 holds them
   * pose_partial_z holds 9 doubles per factor, the entries a form does not use are 0.  PoseTranslationPrior<Pose3> is also the residual
   * and Jacobian of navigation/GPSFactor.cpp:40-43 (p.translation(H) - nT_).  NULL / 0: no such factors.
   * Refused by gtg_upload_problem, each with its own message: an unknown kind; a variable out of range or not POSE3 / POSE2; a noise
   * dimension that is not the row count (3, 3, 2, 1); n_pose_partial > 0 with a table missing.
   * (Appended after the rig-type smart tables: a caller built against the older struct must be recompiled.) */
  int64_t n_pose_partial;
  const int32_t* pose_partial_kind;   /* [n_pose_partial] GTG_POSE_PARTIAL_* */
  const int32_t* pose_partial_var;    /* [n_pose_partial] variable id of the POSE3 or POSE2 */
  const double* pose_partial_z;       /* [n_pose_partial*9] the measurement, see above */
  const int32_t* pose_partial_noise;  /* [n_pose_partial] index into the noise table (dim 3, 3, 2 or 1 by kind and variable type) */

  gtg_planar_table planar;        /* the planar bearing / range factors (GTG_FAC_SAM2): see gtg_planar_table above */
} gtg_problem;
/* pose_partial_kind */
enum { GTG_POSE_PARTIAL_TRANSLATION = 0, GTG_POSE_PARTIAL_ROTATION = 1 };
/* the factor type of the partial pose priors for gtg_get_jacobians (the enum of the factor types above, continued) */
enum { GTG_FAC_POSE_PARTIAL = 6 };
/* ... and of the planar bearing / range factors */
enum { GTG_FAC_SAM2 = 7 };
/* smart_calib[i] of a rig-type smart factor */
enum { GTG_SMART_RIG = -2 };

/* ---- lifetime -------------------------------------------------------------------------------- */
int gtg_create(gtg_handle* out, int device_id);
int gtg_destroy(gtg_handle h);
/* Optional: do the one-time work of the process on `device_id` now (HIP runtime start, code-object load, function objects of every
 * kernel, the factorisation's masked streams) instead of inside the first gtg_create / gtg_upload_problem / gtg_try_lambda.  Idempotent
 * and thread-safe: meant to run on a helper thread while the caller loads or extracts its problem. */
int gtg_prewarm(int device_id);
const char* gtg_last_error(void);
const char* gtg_version(void);

/* One-time symbolic analysis + upload.  Replaces what the reference redoes on EVERY lambda try:
 * VariableIndex (inference/VariableIndex-inl.h:27-49), EliminationTree
 * (EliminationTree-inst.h:77-155), JunctionTree (JunctionTree-inst.h:63-151), Scatter
 * (linear/Scatter.cpp:39-73).  Landmarks (POINT3 touched only by projection / stereo / bearing-range factors / priors) are
 * eliminated first -- the Schur ordering of timing/timeSFMBAL.h:74-83 -- the remaining variables
 * form the reduced system.  shard/n_shards: this handle owns landmark-factors with
 * (landmark rank) % n_shards == shard and other factors with (factor index) % n_shards == shard
 * (multi-GPU); pass 0,1 for a single GPU. */
int gtg_upload_problem(gtg_handle h, const gtg_problem* p, int shard, int n_shards);

/* Optional: position of each non-landmark variable in the reduced system (a fill-reducing
 * ordering, inference/Ordering.cpp:42-124).  order[i] = variable id placed i-th; n = number of
 * non-landmark variables.  Must be called before gtg_upload_problem.  Default: a reverse
 * Cuthill-McKee ordering of the reduced graph computed at upload (band-limits the tile fill). */
int gtg_set_reduced_ordering(gtg_handle h, const int32_t* order, int32_t n);

/* Optional: the camera model of every row of the calib table.  The model does not travel in gtg_problem: a row is a pinhole
 * calibration unless this call says otherwise.  model[k] is the model of calib row k, n_calib the problem's n_calib.  Must be called
 * before gtg_upload_problem; the list is kept by the handle, consumed by the NEXT upload and cleared by it (also by an upload that
 * fails).  NULL or n_calib == 0 clears it.  Without the call, or with every entry GTG_CALIB_PINHOLE, an upload does exactly what it
 * does without it.
 *   GTG_CALIB_FISHEYE: GenericProjectionFactor<Pose3, Point3, Cal3Fisheye> (the equidistant model of geometry/Cal3Fisheye.cpp:47-108):
 *   calib row fx,fy,s,u0,v0 and calib_distortion row k1,k2,k3,k4.  Such a row may be named by monocular projection factors only, in a
 *   graph without stereo, 3-D bearing / range, smart or planar factors; factors with pinhole rows may share the graph.  The upload
 *   refuses everything else, each case with its own message. */
enum { GTG_CALIB_PINHOLE = 0,   /* Cal3_S2, or Cal3DS2 by its calib_distortion row: what every row is without the call */
       GTG_CALIB_FISHEYE = 1 }; /* Cal3Fisheye: calib row fx,fy,s,u0,v0; calib_distortion row k1,k2,k3,k4 */
int gtg_set_calibration_models(gtg_handle h, const int32_t* model, int32_t n_calib);

/* Values in packed storage, variable id order (see GTG_VAR_*).  Values.h:74-79. */
int64_t gtg_values_size(gtg_handle h);   /* doubles in the packed Values (the caller's variables: the landmarks of smart factors are internal) */
int64_t gtg_tangent_size(gtg_handle h);  /* dimension of delta (VectorValues) */
int gtg_set_values(gtg_handle h, const double* packed, int64_t n);
int gtg_get_values(gtg_handle h, double* packed, int64_t n);        /* current (accepted) values */
int gtg_get_trial_values(gtg_handle h, double* packed, int64_t n);  /* values.retract(delta) of the last try */

/* NonlinearFactorGraph::error(values) = sum_i 0.5*||whiten(r_i)||^2
 * (nonlinear/NonlinearFactorGraph.cpp:170-179, NonlinearFactor.cpp:136-147) at the current values. */
int gtg_error(gtg_handle h, double* error);

/* NonlinearFactorGraph::linearize(values) (NonlinearFactorGraph.cpp:239-278) fused with the
 * lambda-invariant part of elimination: J^T J / J^T b block accumulation
 * (JacobianFactor::updateHessian linear/JacobianFactor.cpp:563-598) and
 * GaussianFactorGraph::hessianDiagonal (GaussianFactorGraph.cpp:279-287). */
int gtg_linearize(gtg_handle h);

/* One body of LevenbergMarquardtOptimizer::tryLambda (LevenbergMarquardtOptimizer.cpp:121-270):
 * buildDampedSystem (internal/LevenbergMarquardtState.h:125-156) -> solve
 * (GaussianFactorGraph::optimize, linear/GaussianFactorGraph.cpp:316-319: landmark elimination +
 * Cholesky of the reduced system + back-substitution) -> linear.error(0), linear.error(delta)
 * (GaussianFactorGraph.cpp:71-78) -> values.retract(delta) (nonlinear/Values.cpp:52-63) ->
 * graph.error(newValues).  Returns GTG_OK or GTG_INDETERMINATE; on GTG_OK fills
 *   out[0] = linear.error(0)   out[1] = linear.error(delta)   out[2] = graph.error(trial values)
 *   out[3] = ||delta||_2
 * The trial values stay on the device until gtg_accept(). If linear cost change < 0 the retract /
 * error step is skipped exactly like LM.cpp:178 and out[2] = +inf.
 * Errors (negative return, text in gtg_last_error): a dependency wait of the factorisation ran into its bound (GPU shared or
 * preempted: "the step was not computed" -- never reported as GTG_INDETERMINATE); a smart factor met one of the two cases in
 * which the reference throws (gtg_problem.smart_params; also from gtg_linearize and gtg_error). */
int gtg_try_lambda(gtg_handle h, double lambda, int diagonal_damping, double min_diagonal,
                   double max_diagonal, double out[4]);

/* Same contract as gtg_try_lambda, but the damped reduced system is solved by the reference's preconditioned
 * conjugate gradients (linear/ConjugateGradientSolver.h:106-169; NonlinearOptimizerParams::Iterative with
 * PCGSolverParameters, NonlinearOptimizer.cpp:154-172) with a block-Jacobi preconditioner, applied to the IMPLICIT Schur
 * complement of the landmarks (never formed).  cg = {maxIterations, minIterations, epsilon_rel, epsilon_abs}
 * (ConjugateGradientParameters defaults: 500, 1, 1e-3, 1e-3); *iterations receives the CG iteration count.
 * Single-shard graphs only; not for a planar graph (GTG_VAR_POINT2). */
int gtg_try_lambda_pcg(gtg_handle h, double lambda, int diagonal_damping, double min_diagonal, double max_diagonal,
                       const double cg[4], double out[4], int32_t* iterations);

/* state_ = decreaseLambda(... newValues ...) (LevenbergMarquardtState.h:81-94): trial -> current. */
int gtg_accept(gtg_handle h);

/* Replicated handles -- one per GPU, each holding the WHOLE graph (n_shards = 1), driven in lock step by one process per GPU: the
 * device address of the packed values (which = 0: the current values, 1: the trial values of the last gtg_try_lambda), their
 * length in doubles and the stream the handle's kernels run on, for a device-to-device exchange run by the caller on that stream
 * (e.g. ncclBroadcast of the accepted trial values from the replica whose lambda was taken into every other replica's current
 * values).  After writing a handle's current values in place, gtg_values_changed() tells it so (what gtg_set_values does after
 * its copy): the linearisation and the trial values are no longer valid.  Used by the speculative lambda search of
 * gtsam_amd/speculative.py: replica r tries the r-th lambda of the sequence LevenbergMarquardtOptimizer::tryLambda would walk
 * through on consecutive rejections (LevenbergMarquardtOptimizer.cpp:121-270, LevenbergMarquardtState.h:70-76), the decisions are
 * replayed in order from the gathered results: the trajectory is the sequential one, an iteration costs one try. */
int gtg_values_device_ptr(gtg_handle h, int which, void** ptr, int64_t* n_doubles, void** stream);
int gtg_values_changed(gtg_handle h);

/* ---- parity / debug getters (host copies) --------------------------------------------------- */
int gtg_get_delta(gtg_handle h, double* delta, int64_t n);            /* VectorValues of last solve, variable id order */
int gtg_get_gradient(gtg_handle h, double* g, int64_t n);             /* J^T b, variable id order */
int gtg_get_hessian_diagonal(gtg_handle h, double* d, int64_t n);     /* GaussianFactorGraph::hessianDiagonal */
/* -gradientAtZero() of the caller's linearised graph (GaussianFactorGraph::gradientAtZero, linear/GaussianFactorGraph.cpp), variable id
 * order: gtg_get_gradient, except that every smart factor contributes as the Hessian factor it is in the reference -- its landmark
 * eliminated without damping, so its cameras' blocks are F^T b - F^T E (E^T E)^-1 E^T b (SmartProjectionFactor.h:190-233).  Without
 * smart factors the two getters return the same numbers.  A shard returns the share of its own factors, like gtg_get_gradient. */
int gtg_get_graph_gradient(gtg_handle h, double* g, int64_t n);
/* whitened Jacobian blocks + rhs of factor type `factor_type` after gtg_linearize():
 * row-major per factor: SFM [A1 2x9 | A2 2x3 | b 2], PROJECTION [2x6 | 2x3 | 2],
 * (the caller's own factors: never the measurements of smart factors), BETWEEN [6x6 | 6x6 | 6], PRIOR [d x d | d] padded to d=9 (81+9), STEREO [A1 3x6 | A2 3x3 | b 3] (30 doubles, the caller's stereo
 * factors in the caller's order; PROJECTION keeps returning the 20-double records of the monocular factors alone), SAM the same
 * 30-double record (the caller's bearing / range factors in the caller's order: bearing rows 0-1 and range row 2 of a bearing-range
 * factor, a range-only factor in row 0, a bearing-only factor in rows 0-1; the rows a kind does not use are exactly 0), POSE_PARTIAL the 90-double PRIOR
 * record of the pose's tangent dimension d (the caller's partial pose priors in the caller's order: the factor's 3, 2 or 1 rows first,
 * the rows it does not have exactly 0; PRIOR keeps returning the caller's PriorFactor records alone), SAM2 [A1 3x3 | A2 3x3 | b 3]
 * (21 doubles, the caller's planar bearing / range factors in the caller's order: bearing row 0 and range row 1 of a bearing-range
 * factor, a bearing-only or range-only factor in row 0; A2's third column and the rows a kind does not use are exactly 0).
 * n = doubles available in out. */
int gtg_get_jacobians(gtg_handle h, int factor_type, double* out, int64_t n);
int64_t gtg_reduced_dim(gtg_handle h);
/* dense damped reduced system of the last try: S (n x n row-major, lower triangle valid; after the
 * solve it holds the Cholesky factor L) */
int gtg_get_reduced_matrix(gtg_handle h, double* S, int64_t n_elems);

/* ---- multi-GPU: the one exchange step ------------------------------ */
/* Called by the library with a DEVICE pointer whenever per-shard partial sums must be combined
 * (sum) across shards: reduced Hessian+gradient+scalars.  The callback runs the collective
 * (RCCL all-reduce over xGMI when driven from torch.distributed) and must complete (or be stream
 * ordered on `stream`) before returning. */
typedef int (*gtg_allreduce_fn)(void* device_ptr, int64_t n_doubles, void* stream, void* user);
int gtg_set_allreduce(gtg_handle h, gtg_allreduce_fn fn, void* user);

/* ---- measurement ---------------------------------------------------------------------------- */
/* HIP-event timings (ms, accumulated since the last reset) per phase; names via gtg_phase_name. */
enum { GTG_PH_LINEARIZE = 0, GTG_PH_ASSEMBLE, GTG_PH_POINT_ELIM, GTG_PH_SCHUR, GTG_PH_CHOLESKY,
       GTG_PH_SOLVE, GTG_PH_LINEAR_ERROR, GTG_PH_RETRACT, GTG_PH_ERROR, GTG_PH_COUNT };
int gtg_enable_timing(gtg_handle h, int on);
int gtg_get_phase_ms(gtg_handle h, double* ms, int64_t* calls, int n);
int gtg_reset_timing(gtg_handle h);
const char* gtg_phase_name(int phase);
/* flops of the dense Cholesky factorisation of the last try (n^3/3 + lower order) and the
 * algorithmic HBM bytes of one linearize pass (DESIGN.md section "rooflines") */
double gtg_cholesky_flops(gtg_handle h);
/* the same factorisation counted at the granularity of the variables: sum over the d x d block columns (symbolic fill included)
 * of f^3/3 + f^2 s + f s^2 -- the flops a perfectly sparse elimination would need; gtg_cholesky_flops() counts what the 128x128
 * tile kernels execute (zeros inside stored tiles included) */
double gtg_cholesky_flops_block_level(gtg_handle h);
/* What the dataflow factorisation executes: gtg_cholesky_flops() minus the contraction products it skips because one of their 16 x 16
 * operand sub-tiles is structurally zero (strip-level symbolic factorisation; round 6).  Equal to gtg_cholesky_flops() for the stream
 * schedule and for dense plans. */
double gtg_cholesky_flops_executed(gtg_handle h);
/* identity (63-bit hash) of the layout of the reduced system: elimination order of the reduced variables, their offsets,
 * padding, tile structure and the list of exchanged tiles.  It is derived from the WHOLE graph, so every shard of one job
 * reports the same value; gtg_upload_problem verifies that through the all-reduce callback and fails if they differ. */
int64_t gtg_structure_hash(gtg_handle h);
double gtg_linearize_bytes(gtg_handle h);
/* 1 when some rig-type smart factor of the uploaded graph names a pose key more than once (the kernels that complete the Hessian
 * diagonal and the block-Jacobi blocks on the unique keys are launched for such graphs only), 0 when none does, -1 without a problem.
 * Derived from the WHOLE graph: every shard reports the same value. */
int gtg_smart_repeated_keys(gtg_handle h);
/* doubles of work space the LOST triangulation holds on this handle: 8 per smart measurement of this shard when some smart factor
 * of the graph has useLOST on, 0 otherwise (-1: nothing uploaded) */
int64_t gtg_smart_lost_workspace(gtg_handle h);
/* The TriangulationResult of every smart factor (SmartProjectionFactor::point()) as the last gtg_error / gtg_linearize left it, in
 * the caller's factor order: status[i] = 0 VALID, 1 DEGENERATE, 2 BEHIND_CAMERA, 3 OUTLIER, 4 FAR_POINT, 5 / 6 the two cases in which
 * the reference throws (see smart_params), + 16 when that call replaced the failed track's landmark by a point at infinity;
 * points3[3 i ..] the point (the direction with + 16; zeros for a failed track otherwise).  A track owned by another shard reports
 * status -1 and zeros.  n_smart must be gtg_problem.n_smart. */
int gtg_get_smart_triangulation(gtg_handle h, int32_t* status, double* points3, int64_t n_smart);

/* standalone kernels exposed for unit parity tests (tests/ only): dense FP64 Cholesky of an
 * n x n row-major SPD matrix (lower triangle) held in host memory; returns GTG_INDETERMINATE on a
 * non-positive pivot (Eigen LLT info, base/cholesky.cpp:124-127). */
int gtg_dense_cholesky_host(gtg_handle h, double* A, int32_t n, double* rhs_inout /* may be NULL */);

/* tests only: the tile schedule of the reduced-system Cholesky exactly as the kernels read it (index lists, no numbers), so
 * that the symbolic phase (fill, update lists, elimination-tree parts, backward-solve lists) can be executed and checked
 * on the CPU (tests/test_chol_plan.py).  sizes = {nt, |rows|, |pairs| (int32 entries), |bcols|, n_stored, n_exch, n_pairs
 * of columns, n_parts}; per_tile[nt][4] = trsm_off, trsm_cnt, bwd_off, bwd_cnt; per_pair[np][8] = s1, nar, rest, anc (off, cnt). */
int gtg_debug_plan_sizes(gtg_handle h, int64_t sizes[8]);
int gtg_debug_plan_lists(gtg_handle h, int32_t* rows, int32_t* pairs, int32_t* bcols, int32_t* stored, int32_t* exch,
                         int64_t* per_tile, int64_t* per_pair, int32_t* pair_part, int32_t* part_parent);
/* The dataflow schedule of the same factorisation (csrc/chol_dataflow.hip, the default): sizes = {nt, n_tasks, |klist|, active};
 * tasks[n_tasks][6] = I, J, offset and count into klist, piece r of R (I == J: accumulation of the diagonal tile, I == nt: rhs
 * row; a long contraction is cut into pieces that accumulate in place, the last piece finishes the tile), in the order in which
 * the persistent workgroups take them.  Executed in numpy by tests/test_chol_plan.py. */
int gtg_debug_df_plan(gtg_handle h, int64_t sizes[4], int32_t* tasks, int32_t* klist);
/* The same schedule as the kernels read it, copied back from the device: sizes = {int32 words of the task table (12 per task: the six
 * above, slot of the tile, slot of its diagonal tile, accumulator lanes, first scratch slot, the tile's 64-bit sub-tile mask), words of
 * the step table (6 per contraction step: slots of the two operand tiles, their sub-tile masks), words of the chain table}.  The tables
 * are resolved by a kernel (k_df_resolve) on a real runtime and by a host loop otherwise / with GTG_HOST_SYMBOLIC=1:
 * tests/test_gpu_device_analysis.py compares the two word for word. */
int gtg_debug_df_device_tables(gtg_handle h, int64_t sizes[3], int32_t* tasks, int32_t* steps, int32_t* chain);
/* The diagonal chains of the same schedule: sizes = {chain workgroups W, diagonal tiles, block columns}; workgroup w of the chain
 * kernel factors chain_tiles[chain_off[w] .. chain_off[w + 1]) in that order (one chain = two workgroups that alternate; several
 * chains when a nested-dissection ordering gave the elimination tree independent subtrees -- the reference's parallel elimination of
 * independent cliques, inference/ClusterTree-inst.h:218-317); seq = the order in which the block columns' tasks are queued. */
int gtg_debug_df_chains(gtg_handle h, int64_t sizes[3], int32_t* chain_off, int32_t* chain_tiles, int32_t* seq);
/* The elimination order of the reduced variables the analysis chose (or was given, gtg_set_reduced_ordering): the variable id at
 * every position, n = number of non-landmark variables.  (tests/test_device_analysis_spec.py pins a level-synchronous
 * formulation of the reverse Cuthill-McKee ordering against it.) */
int gtg_debug_reduced_order(gtg_handle h, int32_t* var_of_position, int32_t n);
/* out[0] = tickets taken in the last factorisation; out[8..15] = record of the first dependency wait that gave up (kind 1/2: tile
 * flags of a contraction step, 3: panel of a diagonal tile, 4: accumulated diagonal tile; I, J, k; flag values seen / wanted --
 * out[15], the second wanted value, is replaced by a host counter: the lambda tries of this handle that were repeated with the
 * stream schedule after a time-out of the dataflow pass) */
int gtg_debug_df_ctrl(gtg_handle h, int32_t out[16]);
/* Poll statistics of the dataflow factorisation's dependency waits, counted over the handle's life (round 6): out[0] waits that lasted
 * >= 256 polls, out[1] of those the ones that ended on the read-modify-write poll, out[2] of THOSE the ones whose next ordinary (sc1)
 * load of the same words still returned the old value -- a line the XCD's L2 kept serving --, out[3] / out[4] the same for the shadow
 * words (chol_dataflow.hip::wait_flags; tools/df_stress.py prints them). */
int gtg_debug_df_poll_stats(gtg_handle h, int64_t out[5]);
/* Device memory kept aside for the next handle (released blocks of >= 16 MB, at most GTG_ALLOC_CACHE_MB per device: default 2048,
 * 0 = nothing is kept; the default was 8192 in round 3 and 0 in round 4): give every kept block back to the driver.  Returns the bytes
 * released.  (A failed allocation does this by itself before it gives up.) */
int64_t gtg_release_cached_memory(void);
/* bytes of released device blocks the library currently keeps for the next handle of the process (all devices; GTG_ALLOC_CACHE_MB caps it per device,
 * default 2048, 0 = keep nothing) */
int64_t gtg_cached_memory_bytes(void);
/* GTG_DF_TRACE=1 (read at upload): 100 MHz time stamps of the last factorisation, n = 8 n_tasks + 2 nt: per task {taken,
 * contraction done, done, xcc << 32 | HW_ID, panel 0..3 of the diagonal tile seen}, then per diagonal tile {accumulated tile in, factored} (tools/df_trace.py) */
int gtg_debug_df_trace(gtg_handle h, int64_t* out, int64_t n);

/* tests: the hand-written scan / stable radix sort / run detection of the set-up passes (csrc/primitives.hip) on host arrays.
 * gtg_debug_sort_pairs: key_bytes 4 or 8; val NULL sorts keys only (8-byte keys).  Returns 0, or GTG_ERR_HIP. */
int gtg_debug_scan(int device, const int64_t* in, int64_t n, int64_t* out);
int gtg_debug_sort_pairs(int device, int key_bytes, const void* key, const uint32_t* val, int64_t n, int bits, void* key_out, uint32_t* val_out);
int gtg_debug_runs(int device, const uint64_t* sorted, int64_t n, uint64_t* uniq, int64_t* start, int32_t* n_runs);

/* ---- wire format on the bundle-adjustment side of the path: BAL text files straight to / from the
 * SoA arrays of gtg_problem.  Host-only (no GPU needed).  Replaces SfmData::FromBalFile (gtsam/sfm/SfmData.cpp:189-246: every
 * number goes through a `float`, pose = openGL2gtsam(Rodrigues(w), t), measurement (u, -v), observations grouped by point in
 * file order) and writeBAL (gtsam/sfm/SfmData.cpp:249-327: precision 20, gtsam2openGL, Rot3::Logmap).
 *   cams17  : n_cams x 17 = Pose3 (R row-major 9, t 3) + Cal3Bundler (f, k1, k2, u0, v0)   -- the packed SfmCamera value
 *   points3 : n_points x 3
 *   obs_*   : n_obs observations (camera index, point index, (u, v)), grouped by point
 * Errors: GTG_ERR_USAGE with gtg_io_last_error() (file missing = the reference's runtime_error text). */
const char* gtg_io_last_error(void);
int gtg_io_bal_sizes(const char* path, int64_t* n_cams, int64_t* n_points, int64_t* n_obs);
int gtg_io_read_bal(const char* path, int64_t n_cams, int64_t n_points, int64_t n_obs, double* cams17, double* points3,
                    int32_t* obs_cam, int32_t* obs_point, double* obs_z);
int gtg_io_write_bal(const char* path, int64_t n_cams, int64_t n_points, int64_t n_obs, const double* cams17,
                     const double* points3, const int32_t* obs_cam, const int32_t* obs_point, const double* obs_z);

/* ---- wire formats on the pose-graph side of the path: g2o (VERTEX_SE2 / EDGE_SE2 / VERTEX_SE3:QUAT /
 * EDGE_SE3:QUAT) and TORO (VERTEX2 / EDGE2 / VERTEX3 / EDGE3, also VERTEX / EDGE / ODOMETRY) text files straight to / from the arrays the
 * between-factor tables of gtg_problem are filled from.  Host-only.  Replaces readG2o / load2D / load3D (gtsam/slam/dataset.cpp:505-570,
 * 621-633, 738-944) and writeG2o (:636-735).
 *   is_3d = 1: poses are 12 doubles (R row-major 9, t 3), noise parameters 36 doubles per edge; vertices only where the file lists them
 *              (load3D does not create missing ones);
 *   is_3d = 0: poses are (x, y, theta), noise parameters 9 doubles per edge; `noise_format` says what the six numbers of an edge line
 *              are (readG2o: GTG_IO_NOISE_G2O; load2D's default: GTG_IO_NOISE_AUTO); a vertex an edge refers to and the file does not
 *              list is created along the odometry chain like load2D does;
 *   edge_noise_kind / edge_noise: GTG_NOISE_* + sigma | sigmas | R row-major, the model Gaussian::Information / Covariance(M, smart = true)
 *              returns (linear/NoiseModel.cpp:83-131);  vertices sorted by key (the order gtsam::Values iterates in).
 * gtg_io_write_g2o: VERTEX_* lines of the estimate, then EDGE_* lines with the upper triangle of the information matrix (3-D: in g2o's
 * t,R block order); numbers at the stream's default precision (%g) as writeG2o prints them, or -- full_precision = 1 -- with 17 digits.
 * Errors: GTG_ERR_USAGE with gtg_io_last_error() (file missing = the reference's invalid_argument text). */
enum { GTG_IO_NOISE_AUTO = 0, GTG_IO_NOISE_G2O = 1, GTG_IO_NOISE_TORO = 2, GTG_IO_NOISE_GRAPH = 3, GTG_IO_NOISE_COV = 4 };
int gtg_io_g2o_sizes(const char* path, int is_3d, int noise_format, int64_t* n_edges, int64_t* n_vertices);
int gtg_io_read_g2o(const char* path, int is_3d, int noise_format, int64_t n_edges, int64_t n_vertices, int64_t* edge_v1, int64_t* edge_v2,
                    double* edge_z, int32_t* edge_noise_kind, double* edge_noise, int64_t* vertex_key, double* vertex_pose);
int gtg_io_write_g2o(const char* path, int is_3d, int64_t n_edges, const int64_t* edge_v1, const int64_t* edge_v2, const double* edge_z,
                     const int32_t* edge_noise_kind, const double* edge_noise, int64_t n_vertices, const int64_t* vertex_key,
                     const double* vertex_pose, int full_precision);

#ifdef __cplusplus
}
#endif
#endif /* GTSAM_AMD_H */
