// cRegistration.h -- RANSAC affine fits of matched keypoints, guided matching, subset screening, ZNCC integer search, IC-GN displacement refinement, validation, strain fields and field evaluation (no
// reference counterpart): the steps after enhancedMatch, on the GPU.
// Over sift3d_fit_affine / sift3d_fit_affine_local / sift3d_fit_rigid / sift3d_fit_rigid_local / sift3d_predict_positions / sift3d_match_guided / sift3d_subset_quality / sift3d_zncc_search / sift3d_icgn / sift3d_validate_displacements / sift3d_strain / sift3d_field_eval (include/sift3d_hip.h, which states the numerical contracts).  Both functions take
// exactly the two std::vector<Cvec> that muBruteMatcher::enhancedMatch fills (refMatch[i] <-> tarMatch[i]).
#ifndef S3D_HOST_CREGISTRATION_H
#define S3D_HOST_CREGISTRATION_H

#include <cmath>
#include <vector>

#include "Util/common.h"
#include "cSIFT3D.h"

namespace CPUSIFT {

struct SIFT_LIBRARY_API RansacOptions {
	int iterations = 0;          // hypotheses per problem; 0 = 4096 global, 256 local; at most 65536
	float inlier_thresh = 3.0f;  // tau, in full-resolution voxels
	unsigned seed = 1;
	int refine = 1;              // least-squares refit rounds on the inliers, 0..4
	float min_det = 1.0f;        // a sample (or an inlier covariance) with |det| below this is degenerate
};

// t = L r + b, row-major A = [L | b]; status 0 ok, 1 fewer than 4 candidates, 2 every hypothesis degenerate, 3 refit singular,
// -1 the call failed (message on stderr, like muBruteMatcher)
struct SIFT_LIBRARY_API AffineFit {
	double A[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	double hyp[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // the best minimal-sample hypothesis
	int status = -1;
	int candidates = 0, best_hypothesis = -1, best_count = 0, inliers = 0;
	float rms = 0.f;
	double seconds = 0;  // device time of the call

	// the transform applied to a point, its displacement L p + b - p and the displacement gradient L - I (row-major 3x3)
	Cvec Apply(const Cvec &p) const;
	Cvec Displacement(const Cvec &p) const;
	void Gradient(double G[9]) const;
};

// one fit over all pairs; inlierMask (optional) gets 1 / 0 per pair
SIFT_LIBRARY_API AffineFit EstimateAffine(const std::vector<Cvec> &ref, const std::vector<Cvec> &tar, const RansacOptions &opts = RansacOptions(),
                                          std::vector<int> *inlierMask = nullptr);
// one fit per point (reference coordinates) on its k nearest pairs by reference position (within radius when radius > 0), k in 4..64
SIFT_LIBRARY_API std::vector<AffineFit> EstimateLocalAffine(const std::vector<Cvec> &ref, const std::vector<Cvec> &tar, const std::vector<Cvec> &points,
                                                            int k = 32, float radius = 0, const RansacOptions &opts = RansacOptions());

// Rigid (t = R r + b) and similarity (t = s R r + b) fits over sift3d_fit_rigid / sift3d_fit_rigid_local: the same pairs, options and
// record as the affine fits, with A = hyp = [s R | b].  A fit needs 3 pairs that are not collinear (status 1: fewer than 3), so coplanar
// pairs are fitted; k in 3..64.  RefineDisplacements takes these fits as its init like affine ones.
enum FitModel { Rigid = 0, Similarity = 1 };
SIFT_LIBRARY_API AffineFit EstimateRigid(const std::vector<Cvec> &ref, const std::vector<Cvec> &tar, FitModel model = Rigid,
                                         const RansacOptions &opts = RansacOptions(), std::vector<int> *inlierMask = nullptr);
SIFT_LIBRARY_API std::vector<AffineFit> EstimateLocalRigid(const std::vector<Cvec> &ref, const std::vector<Cvec> &tar, const std::vector<Cvec> &points,
                                                           FitModel model = Rigid, int k = 16, float radius = 0,
                                                           const RansacOptions &opts = RansacOptions());
// the rotation a fit holds (sift3d_fit_rotation, host only): unit quaternion (w, x, y, z; w >= 0), scale and angle in degrees; NaN and
// false for a fit whose status is not 0.  scale and angleDeg may be null.
SIFT_LIBRARY_API bool FitRotation(const AffineFit &fit, double quat[4], double *scale = nullptr, double *angleDeg = nullptr);

// Guided matching over sift3d_predict_positions / sift3d_match_guided: the matcher run again with every reference keypoint's targets
// limited to its gate, the targets within `radius` of its predicted position on each axis (fp32) -- the chain is enhancedMatch ->
// EstimateAffine (or EstimateRigid) -> PredictPositions -> GuidedMatch -> the fit again -> EstimateLocalAffine.  Where texture repeats,
// a keypoint's partner and a look-alike elsewhere in the volume score alike and the ratio test rejects the pair; inside the gate the
// look-alike is not a candidate.
// where a fit sends the keypoints' positions (rx, ry, rz): one fit for all of them, or one per keypoint (EstimateLocalAffine /
// EstimateLocalRigid queried at the keypoints' own positions).  A fit whose status is not 0 gives a NaN position, whose gate is empty;
// so does a failed call (message on stderr)
SIFT_LIBRARY_API std::vector<Cvec> PredictPositions(const AffineFit &fit, const std::vector<Keypoint> &ref_kp);
SIFT_LIBRARY_API std::vector<Cvec> PredictPositions(const std::vector<AffineFit> &fits, const std::vector<Keypoint> &ref_kp);

enum MatchMode { Inject = 1, Biject = 2, Enhanced = 3 };  // muBruteMatcher's injectMatch / bijectMatch / enhancedMatch
// per reference keypoint what muBruteMatcher's getters return after a match (an index negated by a filter, -1 where the gate held no
// usable target) and the number of targets in its gate; ok false: the call failed (message on stderr) and the vectors are empty
struct SIFT_LIBRARY_API GuidedMatchResult {
	std::vector<int> glodenIdx, silverIdx, candidates;
	std::vector<float> glodenDistSquare, silverDistSquare;
	double seconds = 0;  // device time of the call
	bool ok = false;
};
// appends the matched pairs to refMatch / tarMatch as muBruteMatcher does; predicted: one position per reference keypoint; radius in
// (0, 2^20] full-resolution voxels.  A keypoint with one target in its gate is accepted on its distance alone
// (glodenDistSquare / 2 < thresHold^2)
SIFT_LIBRARY_API GuidedMatchResult GuidedMatch(std::vector<Cvec> &refMatch, std::vector<Cvec> &tarMatch, const std::vector<Keypoint> &ref_kp,
                                               const std::vector<Keypoint> &tar_kp, const std::vector<Cvec> &predicted, float radius,
                                               double thresHold = 0.85, MatchMode mode = Enhanced);

struct SIFT_LIBRARY_API IcgnOptions {
	int subset_radius = 16;   // r: the subset is (2r+1)^3 voxels, 2..32
	int max_iterations = 20;  // 1..100
	float tolerance = 1e-3f;  // on ||dp||_r; 0 runs max_iterations updates
	int interpolation = 0;    // 0 tricubic Keys (Catmull-Rom), 1 trilinear, 2 cubic B-spline on the prefiltered target
};

// the refined first-order shape function at one point of interest: p = (u, ux, uy, uz, v, vx, vy, vz, w, wx, wy, wz) (include/sift3d_hip.h);
// status 0 converged, 1 max_iterations reached, 2 subset outside ref, 3 warped subset outside tar, 4 flat subset, 5 init not finite,
// 6 singular step, 7 too few active voxels (RefineDisplacementsMasked only), -1 the call failed (message on stderr, like EstimateAffine)
struct SIFT_LIBRARY_API IcgnResult {
	double p[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	double zncc = 0, last_step = 0;
	int iterations = 0;
	int status = -1;
	double seconds = 0;  // device time of the call

	// (u, v, w) and the displacement gradient (row-major 3x3: rows u, v, w; columns x, y, z)
	Cvec Displacement() const;
	void Gradient(double G[9]) const;
};

struct SIFT_LIBRARY_API SearchOptions {
	int subset_radius = 8;  // r: the subset is (2r+1)^3 voxels, 2..16
	int search_radius = 8;  // s: candidates are guess + [-s, s]^3, 1..16
};

// the integer displacement of highest ZNCC at one point of interest (include/sift3d_hip.h); status 0 found, 2 subset outside ref,
// 3 no candidate scored (d = the guess), 4 flat subset, -1 the call failed (message on stderr, like EstimateAffine)
struct SIFT_LIBRARY_API SearchResult {
	int d[3] = {0, 0, 0};
	int status = -1;
	double zncc = 0, zncc_second = -2.0;  // at d; the best score at Chebyshev distance > 1 from d (-2: none)
	int candidates = 0;                   // candidates scored
	double seconds = 0;                   // device time of the call

	Cvec Displacement() const;
};

// exhaustive integer search of the displacement from ref to tar at integral points of ref, around the guesses (integral, one per
// point) or around zero: the initial guess of RefineDisplacements where no local fit exists
SIFT_LIBRARY_API std::vector<SearchResult> SearchDisplacements(const float *ref, int nx, int ny, int nz, const float *tar, int tnx, int tny, int tnz,
                                                               const std::vector<Cvec> &points, const std::vector<Cvec> *guesses = nullptr,
                                                               const SearchOptions &o = SearchOptions());

struct SIFT_LIBRARY_API SubsetOptions {
	int r_min = 8, r_max = 16;  // the radii walked, 2 <= r_min <= r_max <= 32
	int criterion = 0;          // 0 min(Gxx, Gyy, Gzz), the per-axis SSSIG; 1 the smallest eigenvalue of G
	double threshold = 0;       // the criterion a subset must reach (2 sigma_noise^2 / sigma_u^2); 0 accepts r_min everywhere
	double level = -INFINITY;   // a voxel is material when its value is >= level
	double fraction_min = 0;    // the fraction of material voxels a subset must hold, 0..1
};

// the texture sums of the subset around one point of interest and its radius (include/sift3d_hip.h); status 0 the radius qualifies,
// 1 no radius does (the record is that of `feasible`), 2 the cube of r_min leaves ref, 3 too little material, -1 the call failed
// (message on stderr, like EstimateAffine)
struct SIFT_LIBRARY_API SubsetQuality {
	double mean = 0, dR = 0;
	double G[6] = {0, 0, 0, 0, 0, 0};  // xx yy zz xy xz yz
	double eig[3] = {0, 0, 0};         // of G, descending
	int radius = 0;
	int status = -1;
	int feasible = 0, material = 0;
	double seconds = 0;                // device time of the call
};

// the step in front of RefineDisplacements: per integral point of ref the smallest subset radius of o.r_min .. o.r_max whose texture
// reaches o.threshold, or that none does
SIFT_LIBRARY_API std::vector<SubsetQuality> SelectSubsets(const float *ref, int nx, int ny, int nz, const std::vector<Cvec> &points,
                                                          const SubsetOptions &o = SubsetOptions());
// the indices of the status-0 records grouped by radius: groups[r - r_min] lists, in ascending order, the points whose subset has radius
// r -- one RefineDisplacements call per non-empty group with IcgnOptions::subset_radius = r.  false: a bad range, or a status-0 radius
// outside it (message on stderr)
SIFT_LIBRARY_API bool GroupSubsetsByRadius(const std::vector<SubsetQuality> &quality, int r_min, int r_max, std::vector<std::vector<int>> &groups);

// the cubic B-spline coefficients (mirror boundary) of vol (nx x ny x nz, fp32, x fastest) into coefficients, host memory of the same
// size and not vol itself: what RefineDisplacements takes as tar with interpolation 2 and tar_is_coefficients, so a target refined
// against more than once is prefiltered once.  false: the call failed (message on stderr).  seconds (may be null): device time
SIFT_LIBRARY_API bool PrefilterBSpline(const float *vol, int nx, int ny, int nz, float *coefficients, double *seconds = nullptr);

// vol (nx x ny x nz voxels of `type`, host memory, x fastest) as an fp32 volume in d_dst, DEVICE memory of nx * ny * nz floats on the
// selected GPU (SetDevice) that the caller owns: the shell's name for sift3d_volume_to_device (include/sift3d_hip.h).  The volume
// travels through the pinned staging pool at its own width and 8 / 16-bit integers are widened on the GPU; d_dst is complete on
// return and is what the on_device forms of the C-ABI (sift3d_icgn, sift3d_zncc_search, ...) take, uploaded once for many calls.
// false: the call failed (message on stderr).  seconds (may be null): device time of the widening kernel
SIFT_LIBRARY_API bool UploadVolume(const void *vol, VoxelType type, int nx, int ny, int nz, float *d_dst, double *seconds = nullptr);

// IC-GN refinement of the displacement from ref (nx x ny x nz, fp32, x fastest) to tar (tnx x tny x tnz) at integral points of ref,
// starting from the local affine fits (one per point, e.g. EstimateLocalAffine at the same points) or from zero; fallback (one per
// point, e.g. SearchDisplacements at the same points) gives the start of a point whose fit has status != 0.  opts.interpolation 2
// interpolates tar by cubic B-splines: tar is prefiltered inside the call, or, with tar_is_coefficients, already holds
// PrefilterBSpline's output, through the second overload (the flag has no meaning for the interpolations 0 and 1).  The first
// overload is the function as it was: programs linked against an earlier libsift3d.so still resolve it
SIFT_LIBRARY_API std::vector<IcgnResult> RefineDisplacements(const float *ref, int nx, int ny, int nz, const float *tar, int tnx, int tny, int tnz,
                                                             const std::vector<Cvec> &points, const std::vector<AffineFit> *init = nullptr,
                                                             const IcgnOptions &opts = IcgnOptions(),
                                                             const std::vector<SearchResult> *fallback = nullptr);
SIFT_LIBRARY_API std::vector<IcgnResult> RefineDisplacements(const float *ref, int nx, int ny, int nz, const float *tar, int tnx, int tny, int tnz,
                                                             const std::vector<Cvec> &points, const std::vector<AffineFit> *init,
                                                             const IcgnOptions &opts, const std::vector<SearchResult> *fallback,
                                                             bool tar_is_coefficients);

// mask (nx x ny x nz bytes, host memory, x fastest) = 1 where vol >= level, else 0 (a NaN voxel is 0): SelectSubsets' rule for a material
// voxel, and the mask RefineDisplacementsMasked takes.  false: the call failed (message on stderr).  seconds (may be null): device time
SIFT_LIBRARY_API bool MaskFromLevel(const float *vol, int nx, int ny, int nz, double level, unsigned char *mask, double *seconds = nullptr);

// RefineDisplacements at a specimen's surface, at pores and cracks and where two bodies touch: every sum of the correlation runs over
// the active voxels of the subset only -- those that, with their six face neighbours, are in mask (one byte per voxel of ref, any
// non-zero byte is "in"; include/sift3d_hip.h, sift3d_icgn_masked).  A point whose subset holds no active voxel, or fewer than
// min_fraction (0..1) of its (2r+1)^3, returns status 7.  init: one local affine fit per point or null (zero); opts.interpolation 0, 1
// or 2, tar_is_coefficients as for RefineDisplacements (interpolation 2 only).  active (may be null): resized to one count of active
// voxels per point
SIFT_LIBRARY_API std::vector<IcgnResult> RefineDisplacementsMasked(const float *ref, int nx, int ny, int nz, const float *tar, int tnx, int tny,
                                                                   int tnz, const unsigned char *mask, const std::vector<Cvec> &points,
                                                                   const std::vector<AffineFit> *init = nullptr,
                                                                   const IcgnOptions &opts = IcgnOptions(), float min_fraction = 0.f,
                                                                   std::vector<int> *active = nullptr, bool tar_is_coefficients = false);

// the refined second-order shape function at one point of interest: p = (c, cx, cy, cz, cxx, cyy, czz, cxy, cxz, cyz) of u, then v, then w
// -- the displacement and its first and second derivatives at the point (include/sift3d_hip.h); status as IcgnResult's
struct SIFT_LIBRARY_API Icgn2Result {
	double p[30] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	double zncc = 0, last_step = 0;
	int iterations = 0;
	int status = -1;
	double seconds = 0;  // device time of the call

	// (u, v, w), the displacement gradient (row-major 3x3: rows u, v, w; columns x, y, z) and the second derivatives (row-major 3x6:
	// rows u, v, w; columns xx, yy, zz, xy, xz, yz)
	Cvec Displacement() const;
	void Gradient(double G[9]) const;
	void SecondDerivatives(double S[18]) const;
};

// second-order IC-GN at integral points of ref, started from the first-order results at the same points (RefineDisplacements): a point
// whose first-order status is 0 or 1 starts from its 12 parameters with zero second derivatives, any other point returns status 5.
// Removes the bias of the first-order fit where the displacement gradient varies across the subset.  opts.interpolation 0, 1 or 2;
// tar_is_coefficients as for RefineDisplacements (interpolation 2 only)
SIFT_LIBRARY_API std::vector<Icgn2Result> RefineDisplacementsSecondOrder(const float *ref, int nx, int ny, int nz, const float *tar, int tnx, int tny,
                                                                         int tnz, const std::vector<Cvec> &points,
                                                                         const std::vector<IcgnResult> &first,
                                                                         const IcgnOptions &opts = IcgnOptions(), bool tar_is_coefficients = false);

struct SIFT_LIBRARY_API StrainOptions {
	int radius = 16;          // window half width in voxels (Chebyshev), 1..4096
	int min_neighbours = 10;  // 4..1048576
	int measure = 0;          // 0 Green-Lagrange, 1 infinitesimal
};

// the plane fitted to the displacements of the points within `radius` of one point of interest and its strain (include/sift3d_hip.h);
// status 0 fitted, 1 fewer than min_neighbours neighbours, 2 coordinate out of range, 4 degenerate window (coplanar neighbours),
// -1 the call failed (message on stderr, like EstimateAffine)
struct SIFT_LIBRARY_API StrainResult {
	double disp[3] = {0, 0, 0};                    // fitted displacement at the point
	double G[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};     // fitted gradient, row-major: rows u, v, w; columns x, y, z
	double E[6] = {0, 0, 0, 0, 0, 0};              // xx yy zz xy yz zx
	double principal[3] = {0, 0, 0};               // eigenvalues of E, descending
	double equivalent = 0, rms = 0;
	int neighbours = 0;
	int status = -1;
	double seconds = 0;  // device time of the call
};

// strain at every point from the displacements RefineDisplacements returned at the same points: a point is a neighbour where IC-GN
// converged (or ran out of iterations, with accept_unconverged) with zncc >= zncc_min; the others are filled from their neighbours
SIFT_LIBRARY_API std::vector<StrainResult> ComputeStrains(const std::vector<Cvec> &points, const std::vector<IcgnResult> &disp,
                                                          const StrainOptions &o = StrainOptions(), double zncc_min = 0,
                                                          bool accept_unconverged = false);
// the same from the second-order results of RefineDisplacementsSecondOrder
SIFT_LIBRARY_API std::vector<StrainResult> ComputeStrains(const std::vector<Cvec> &points, const std::vector<Icgn2Result> &disp,
                                                          const StrainOptions &o = StrainOptions(), double zncc_min = 0,
                                                          bool accept_unconverged = false);

struct SIFT_LIBRARY_API ValidationOptions {
	int radius = 16;         // window half width in voxels (Chebyshev), 1..4096
	int min_neighbours = 6;  // fewest neighbours a tested point may have, 3..1048576
	int passes = 2;          // 1..8
	double threshold = 2.0;  // a score above this flags the point
	double eps = 0.1;        // noise floor in voxels added to the MAD
};

// the normalised median test of one point's displacement against its neighbours' (include/sift3d_hip.h): status 0 tested, 1 fewer than
// min_neighbours neighbours, 2 coordinate out of range, 3 the point does not contribute (median and mad are the neighbours': the value
// that fills the hole), -1 the call failed (message on stderr, like EstimateAffine).  flagged and pass come from the passes and are
// authoritative, whatever the final score
struct SIFT_LIBRARY_API ValidationResult {
	double median[3] = {0, 0, 0}, mad[3] = {0, 0, 0};
	double score = 0;
	int neighbours = 0;
	int status = -1;
	int flagged = 0, pass = 0;
	double seconds = 0;  // device time of the call
};

// outlier test of the displacements RefineDisplacements returned at the same points, between IC-GN and ComputeStrains: a point
// contributes under ComputeStrains' rule (zncc_min, accept_unconverged); use_gradients carries a neighbour's value to the tested point
// with the neighbour's own IC-GN gradient, which keeps strongly deforming fields clear of false alarms
SIFT_LIBRARY_API std::vector<ValidationResult> ValidateDisplacements(const std::vector<Cvec> &points, const std::vector<IcgnResult> &disp,
                                                                     const ValidationOptions &o = ValidationOptions(), double zncc_min = 0,
                                                                     bool accept_unconverged = false, bool use_gradients = true);
SIFT_LIBRARY_API std::vector<ValidationResult> ValidateDisplacements(const std::vector<Cvec> &points, const std::vector<Icgn2Result> &disp,
                                                                     const ValidationOptions &o = ValidationOptions(), double zncc_min = 0,
                                                                     bool accept_unconverged = false, bool use_gradients = true);
// one byte per point: 1 where the point was tested (status 0) and not flagged -- what the ComputeStrains overloads below take as keep
SIFT_LIBRARY_API std::vector<unsigned char> KeepMask(const std::vector<ValidationResult> &validation);
// ComputeStrains with a point contributing only where keep is non-zero as well (keep: one byte per point)
SIFT_LIBRARY_API std::vector<StrainResult> ComputeStrains(const std::vector<Cvec> &points, const std::vector<IcgnResult> &disp,
                                                          const std::vector<unsigned char> &keep, const StrainOptions &o = StrainOptions(),
                                                          double zncc_min = 0, bool accept_unconverged = false);
SIFT_LIBRARY_API std::vector<StrainResult> ComputeStrains(const std::vector<Cvec> &points, const std::vector<Icgn2Result> &disp,
                                                          const std::vector<unsigned char> &keep, const StrainOptions &o = StrainOptions(),
                                                          double zncc_min = 0, bool accept_unconverged = false);
// starts of a second RefineDisplacements (its init) from a first one and its validation: a point that was flagged (status 0), or that
// did not contribute (status 3), restarts from its neighbours' median, A = [I | median], status 0; a kept point (tested, not flagged)
// from the affine map of its own result, L = I + G and b with L q + b - q = u, status 0; any other point gets status 1 (no start)
SIFT_LIBRARY_API std::vector<AffineFit> SeedsFromValidation(const std::vector<Cvec> &points, const std::vector<IcgnResult> &first,
                                                            const std::vector<ValidationResult> &validation);

struct SIFT_LIBRARY_API FieldOptions {
	int radius = 16;               // window half width in voxels (Chebyshev), 1..4095
	int min_neighbours = 10;       // 4..1048576
	int weighting = 1;             // 1 tensor biweight, 0 uniform
	bool require_enclosed = true;  // status 5 unless the query has neighbours on both sides of every axis
};

// the displacement field at one real-valued position (include/sift3d_hip.h, sift3d_field_eval): status 0 fitted, 1 fewer than
// min_neighbours neighbours, 2 position not finite or out of range, 4 degenerate window, 5 not enclosed, -1 the call failed (message on
// stderr, like EstimateAffine) or, from ComposeDisplacements, no value
struct SIFT_LIBRARY_API FieldResult {
	double disp[3] = {0, 0, 0};                 // the field at the position
	double G[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // its gradient, row-major: rows u, v, w; columns x, y, z
	double rms = 0, wsum = 0;
	int neighbours = 0, sides = 0;
	int status = -1;
	double seconds = 0;  // device time of the call
};

// the field of the displacements RefineDisplacements returned at `points`, evaluated at the positions queries3 (x, y, z triples): a
// point contributes under ComputeStrains' rule (zncc_min, accept_unconverged)
SIFT_LIBRARY_API std::vector<FieldResult> EvaluateField(const std::vector<Cvec> &points, const std::vector<IcgnResult> &disp,
                                                        const std::vector<double> &queries3, const FieldOptions &o = FieldOptions(),
                                                        double zncc_min = 0, bool accept_unconverged = false);
// the same at the positions the points of an earlier load step moved to, p + u_A(p): the second step of a load series with an updated
// reference.  A point of step A whose displacement is not finite gets status 2
SIFT_LIBRARY_API std::vector<FieldResult> EvaluateField(const std::vector<Cvec> &points, const std::vector<IcgnResult> &disp,
                                                        const std::vector<Cvec> &pointsA, const std::vector<IcgnResult> &stepA,
                                                        const FieldOptions &o = FieldOptions(), double zncc_min = 0,
                                                        bool accept_unconverged = false);
// the total of two load steps in step A's frame: disp = u_A + u_B, G = G_A + G_B + G_B G_A, status 0 where step A converged (status 0)
// and atB -- EvaluateField at the moved points -- has status 0; -1 (all zero) elsewhere, or everywhere when the sizes differ
SIFT_LIBRARY_API std::vector<FieldResult> ComposeDisplacements(const std::vector<IcgnResult> &stepA, const std::vector<FieldResult> &atB);
// starts of RefineDisplacements (its init) at `points` from a field evaluated or composed there: A = [I + G | b] with
// (I + G) q + b - q = u, status 0 where the field's status is 0; status 1 (no start) elsewhere
SIFT_LIBRARY_API std::vector<AffineFit> SeedsFromField(const std::vector<Cvec> &points, const std::vector<FieldResult> &field);

// ---- several bodies: labels (include/sift3d_hip.h, sift3d_mask_label and the labelled window calls) ---------------------------------
// labels (nx x ny x nz ints, host memory, x fastest): 0 where mask is 0, else the number 1..*count of the voxel's connected component
// (connectivity 6: faces; 26: faces, edges and corners), numbered in ascending order of a component's lowest voxel; a component of fewer
// than min_voxels voxels gets 0 and is not counted.  false: the call failed (message on stderr).  seconds (may be null): device time.
// The mask of body L for RefineDisplacementsMasked is labels == L.
SIFT_LIBRARY_API bool LabelMask(const unsigned char *mask, int nx, int ny, int nz, int connectivity, int min_voxels, int *labels, int *count,
                                double *seconds = nullptr);
// the label at each point (0 for a point outside the volume); host only.  Empty when a coordinate is not integral
SIFT_LIBRARY_API std::vector<int> LabelsAt(const int *labels, int nx, int ny, int nz, const std::vector<Cvec> &points);
// ---- bodies that touch (include/sift3d_hip.h, sift3d_mask_distance and sift3d_mask_split) ----------------------------------------------
// dist2 (nx x ny x nz ints, host memory): the exact squared Euclidean distance of every in-voxel of mask to the nearest out-voxel, 0
// for an out-voxel.  border: the layer of voxels around the volume counts as out; without it and without an out-voxel every entry is
// SIFT3D_DIST2_NONE.  false: the call failed (message on stderr).  seconds (may be null): device time.
SIFT_LIBRARY_API bool DistanceTransform(const unsigned char *mask, int nx, int ny, int nz, bool border, int *dist2, double *seconds = nullptr);
// mask = dist2 >= level2: with level2 >= 1 the exact erosion by the open ball of squared radius level2 of the mask DistanceTransform saw
SIFT_LIBRARY_API bool ErodeMask(const int *dist2, int nx, int ny, int nz, int level2, unsigned char *mask, double *seconds = nullptr);
// dist2 at each point (0 for a point outside the volume): the squared distance of a point to its body's surface; host only.  Empty when
// a coordinate is not integral
SIFT_LIBRARY_API std::vector<int> DistancesAt(const int *dist2, int nx, int ny, int nz, const std::vector<Cvec> &points);
struct SplitOptions {
	int connectivity = 6;     // 6 or 26: of the cores' components and of the growth
	int core_dist2 = 16;      // a core voxel has dist2 >= core_dist2: above the squared half-width of the widest neck between two grains,
	                          // at most the squared inradius of the smallest grain to keep apart
	int min_core_voxels = 1;  // smaller cores seed nothing
	bool border = true;       // as DistanceTransform
	int max_rounds = 0;       // growth rounds at most; 0: until a round labels nothing
	bool keep_unreached = true;  // the components no core reaches become bodies too, numbered behind the cores
	int min_voxels = 1;       // size cut of those components
};
struct SplitInfo {
	int cores = 0, unreached_bodies = 0, rounds = 0, unlabelled = 0;
};
// LabelMask for bodies that touch: the components of dist2 >= core_dist2 are numbered as LabelMask numbers them and grown back over the
// mask in synchronous rounds, a voxel taking the label of its labelled neighbour with the largest dist2 (ties: the smallest label).  A
// grain too small to hold a core is a body of its own only where it stands alone; one that touches a grain with a core is absorbed.
// dist2 (may be null): the transform; info (may be null).  false: the call failed (message on stderr)
SIFT_LIBRARY_API bool SplitBodies(const unsigned char *mask, int nx, int ny, int nz, int *labels, int *count,
                                  const SplitOptions &o = SplitOptions(), int *dist2 = nullptr, SplitInfo *info = nullptr,
                                  double *seconds = nullptr);
// One rigid (or similarity) fit per body of a labelled specimen (include/sift3d_hip.h, sift3d_fit_rigid_bodies): every matched pair is
// given the label at the voxel nearest to its reference position (0 outside the volume) and body L = 1..count is fitted from its own
// pairs alone; the result holds `count` fits, body L at index L - 1 (status 1: fewer than 3 pairs).  pairLabels (may be null): resized
// to one label per pair; inlierMask (may be null): resized to one entry per pair, 1 where the pair is an inlier of its own body's fit.
// opts.iterations 0 means 256.  Empty when the call failed (message on stderr).
SIFT_LIBRARY_API std::vector<AffineFit> EstimateBodyRigid(const std::vector<Cvec> &ref, const std::vector<Cvec> &tar, const int *labels, int nx,
                                                          int ny, int nz, int count, FitModel model = Rigid,
                                                          const RansacOptions &opts = RansacOptions(), std::vector<int> *pairLabels = nullptr,
                                                          std::vector<int> *inlierMask = nullptr);
// starts of RefineDisplacements / RefineDisplacementsLabelled (their init) at `points`: the fit of the body each point lies in
// (pointLabels: what LabelsAt returns; fits: what EstimateBodyRigid returns); a point of no body gets status 1 (no start)
SIFT_LIBRARY_API std::vector<AffineFit> SeedsFromBodyFits(const std::vector<AffineFit> &fits, const std::vector<int> &pointLabels);
// RefineDisplacementsMasked with every point limited to its own body, in one call: point i is treated as under the mask
// labels == labels[point i] (include/sift3d_hip.h, sift3d_icgn_labelled); a point on a voxel whose label is <= 0 returns status 7.
// active, pointLabels (may be null): resized to one count of active voxels and one label per point
SIFT_LIBRARY_API std::vector<IcgnResult> RefineDisplacementsLabelled(const float *ref, int nx, int ny, int nz, const float *tar, int tnx, int tny,
                                                                     int tnz, const int *labels, const std::vector<Cvec> &points,
                                                                     const std::vector<AffineFit> *init = nullptr,
                                                                     const IcgnOptions &opts = IcgnOptions(), float min_fraction = 0.f,
                                                                     std::vector<int> *active = nullptr, std::vector<int> *pointLabels = nullptr,
                                                                     bool tar_is_coefficients = false);
// ComputeStrains, ValidateDisplacements and EvaluateField limited to a point's own body: a point is a neighbour of another only where
// both have the same label > 0 (labels: one per point, what LabelsAt returns); a point or query whose label is <= 0 gets status 1 with no
// neighbours.  keep (may be null): as for ComputeStrains with keep.  query_labels: one per query
SIFT_LIBRARY_API std::vector<StrainResult> ComputeStrains(const std::vector<Cvec> &points, const std::vector<IcgnResult> &disp,
                                                          const std::vector<int> &labels, const std::vector<unsigned char> *keep = nullptr,
                                                          const StrainOptions &o = StrainOptions(), double zncc_min = 0,
                                                          bool accept_unconverged = false);
SIFT_LIBRARY_API std::vector<StrainResult> ComputeStrains(const std::vector<Cvec> &points, const std::vector<Icgn2Result> &disp,
                                                          const std::vector<int> &labels, const std::vector<unsigned char> *keep = nullptr,
                                                          const StrainOptions &o = StrainOptions(), double zncc_min = 0,
                                                          bool accept_unconverged = false);
SIFT_LIBRARY_API std::vector<ValidationResult> ValidateDisplacements(const std::vector<Cvec> &points, const std::vector<IcgnResult> &disp,
                                                                     const std::vector<int> &labels,
                                                                     const ValidationOptions &o = ValidationOptions(), double zncc_min = 0,
                                                                     bool accept_unconverged = false, bool use_gradients = true);
SIFT_LIBRARY_API std::vector<ValidationResult> ValidateDisplacements(const std::vector<Cvec> &points, const std::vector<Icgn2Result> &disp,
                                                                     const std::vector<int> &labels,
                                                                     const ValidationOptions &o = ValidationOptions(), double zncc_min = 0,
                                                                     bool accept_unconverged = false, bool use_gradients = true);
SIFT_LIBRARY_API std::vector<FieldResult> EvaluateField(const std::vector<Cvec> &points, const std::vector<IcgnResult> &disp,
                                                        const std::vector<int> &labels, const std::vector<double> &queries3,
                                                        const std::vector<int> &query_labels, const FieldOptions &o = FieldOptions(),
                                                        double zncc_min = 0, bool accept_unconverged = false);

}  // namespace CPUSIFT
#endif
