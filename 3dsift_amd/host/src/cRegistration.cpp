// cRegistration.cpp -- CPUSIFT::EstimateAffine / EstimateLocalAffine / PredictPositions / GuidedMatch / SearchDisplacements / RefineDisplacements / RefineDisplacementsMasked / RefineDisplacementsLabelled / EstimateBodyRigid / SeedsFromBodyFits / MaskFromLevel / ValidateDisplacements /
// ComputeStrains over sift3d_fit_affine / sift3d_fit_affine_local / sift3d_predict_positions / sift3d_match_guided / sift3d_zncc_search / sift3d_icgn / sift3d_icgn_bspline / sift3d_icgn_masked /
// sift3d_mask_from_level / sift3d_validate_displacements / sift3d_strain, CPUSIFT::LabelMask / LabelsAt and the labelled overloads over
// sift3d_mask_label / sift3d_labels_at_points / sift3d_*_labelled, and
// CPUSIFT::PrefilterBSpline over sift3d_bspline_prefilter (include/sift3d_hip.h).
#include "../Include/cRegistration.h"

#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../../include/sift3d_hip.h"

namespace CPUSIFT {

namespace {
sift3d_ransac_options to_c(const RansacOptions &o) {
	sift3d_ransac_options c;
	sift3d_default_ransac_options(&c);
	c.iterations = o.iterations;
	c.inlier_thresh = o.inlier_thresh;
	c.seed = o.seed;
	c.refine = o.refine;
	c.min_det = o.min_det;
	return c;
}
void from_c(const sift3d_affine_fit &f, double sec, AffineFit &a) {
	memcpy(a.A, f.A, sizeof(a.A));
	memcpy(a.hyp, f.hyp, sizeof(a.hyp));
	a.status = f.status;
	a.candidates = f.candidates;
	a.best_hypothesis = f.best_hypothesis;
	a.best_count = f.best_count;
	a.inliers = f.inliers;
	a.rms = f.rms;
	a.seconds = sec;
}
std::vector<float> pairs6(const std::vector<Cvec> &ref, const std::vector<Cvec> &tar, size_t n) {
	std::vector<float> p(6 * (n ? n : 1));
	for (size_t i = 0; i < n; i++) {
		p[6 * i] = ref[i].x; p[6 * i + 1] = ref[i].y; p[6 * i + 2] = ref[i].z;
		p[6 * i + 3] = tar[i].x; p[6 * i + 4] = tar[i].y; p[6 * i + 5] = tar[i].z;
	}
	return p;
}
// points with integral coordinates -> int triples; false (message on stderr) when one is not integral
bool int_triples(const char *who, const char *what, const std::vector<Cvec> &points, std::vector<int> &q) {
	const size_t m = points.size();
	q.assign(3 * (m ? m : 1), 0);
	for (size_t i = 0; i < m; i++) {
		const float c[3] = {points[i].x, points[i].y, points[i].z};
		for (int a = 0; a < 3; a++) {
			if (!(std::floor(c[a]) == c[a]) || std::fabs(c[a]) > 2e9f) {
				fprintf(stderr, "[3dsift_amd] %s: %s %zu is not an integral voxel\n", who, what, i);
				return false;
			}
			q[3 * i + a] = (int)c[a];
		}
	}
	return true;
}
}  // namespace

Cvec AffineFit::Apply(const Cvec &p) const {
	double v[3];
	for (int i = 0; i < 3; i++) v[i] = A[4 * i] * p.x + A[4 * i + 1] * p.y + A[4 * i + 2] * p.z + A[4 * i + 3];
	return Cvec((float)v[0], (float)v[1], (float)v[2]);
}
Cvec AffineFit::Displacement(const Cvec &p) const {
	const Cvec t = Apply(p);
	return Cvec(t.x - p.x, t.y - p.y, t.z - p.z);
}
void AffineFit::Gradient(double G[9]) const {
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 3; j++) G[3 * i + j] = A[4 * i + j] - (i == j ? 1.0 : 0.0);
}

namespace {
// the global fit of one model (-1: affine)
AffineFit estimate_global(const char *who, int model, const std::vector<Cvec> &ref, const std::vector<Cvec> &tar, const RansacOptions &opts,
                          std::vector<int> *inlierMask) {
	AffineFit a;
	const size_t n = ref.size() < tar.size() ? ref.size() : tar.size();
	const std::vector<float> p = pairs6(ref, tar, n);
	const sift3d_ransac_options o = to_c(opts);
	std::vector<unsigned char> mask(n ? n : 1);
	sift3d_affine_fit f;
	double sec = 0;
	const int rc = model < 0 ? sift3d_fit_affine(p.data(), (int)n, &o, 0, GetDevice(), &f, mask.data(), &sec)
	                         : sift3d_fit_rigid(p.data(), (int)n, model, &o, 0, GetDevice(), &f, mask.data(), &sec);
	if (rc != SIFT3D_OK) {
		fprintf(stderr, "[3dsift_amd] %s: %s (%s)\n", who, sift3d_error_string(rc), sift3d_last_error());
		if (inlierMask) inlierMask->assign(n, 0);
		return a;
	}
	from_c(f, sec, a);
	if (inlierMask) inlierMask->assign(mask.begin(), mask.begin() + n);
	return a;
}

// the local fits of one model (-1: affine)
std::vector<AffineFit> estimate_local(const char *who, int model, const std::vector<Cvec> &ref, const std::vector<Cvec> &tar,
                                      const std::vector<Cvec> &points, int k, float radius, const RansacOptions &opts) {
	const size_t n = ref.size() < tar.size() ? ref.size() : tar.size(), m = points.size();
	std::vector<AffineFit> res(m);
	const std::vector<float> p = pairs6(ref, tar, n);
	std::vector<float> q(3 * (m ? m : 1));
	for (size_t i = 0; i < m; i++) { q[3 * i] = points[i].x; q[3 * i + 1] = points[i].y; q[3 * i + 2] = points[i].z; }
	const sift3d_ransac_options o = to_c(opts);
	std::vector<sift3d_affine_fit> f(m ? m : 1);
	double sec = 0;
	const int rc = model < 0 ? sift3d_fit_affine_local(p.data(), (int)n, q.data(), (int)m, k, radius, &o, 0, GetDevice(), f.data(), nullptr, &sec)
	                         : sift3d_fit_rigid_local(p.data(), (int)n, q.data(), (int)m, k, radius, model, &o, 0, GetDevice(), f.data(), nullptr, &sec);
	if (rc != SIFT3D_OK) {
		fprintf(stderr, "[3dsift_amd] %s: %s (%s)\n", who, sift3d_error_string(rc), sift3d_last_error());
		return res;
	}
	for (size_t i = 0; i < m; i++) from_c(f[i], sec, res[i]);
	return res;
}
}  // namespace

AffineFit EstimateAffine(const std::vector<Cvec> &ref, const std::vector<Cvec> &tar, const RansacOptions &opts, std::vector<int> *inlierMask) {
	return estimate_global("EstimateAffine", -1, ref, tar, opts, inlierMask);
}

std::vector<AffineFit> EstimateLocalAffine(const std::vector<Cvec> &ref, const std::vector<Cvec> &tar, const std::vector<Cvec> &points, int k, float radius,
                                           const RansacOptions &opts) {
	return estimate_local("EstimateLocalAffine", -1, ref, tar, points, k, radius, opts);
}

AffineFit EstimateRigid(const std::vector<Cvec> &ref, const std::vector<Cvec> &tar, FitModel model, const RansacOptions &opts,
                        std::vector<int> *inlierMask) {
	return estimate_global("EstimateRigid", (int)model, ref, tar, opts, inlierMask);
}

std::vector<AffineFit> EstimateLocalRigid(const std::vector<Cvec> &ref, const std::vector<Cvec> &tar, const std::vector<Cvec> &points, FitModel model,
                                          int k, float radius, const RansacOptions &opts) {
	return estimate_local("EstimateLocalRigid", (int)model, ref, tar, points, k, radius, opts);
}

bool FitRotation(const AffineFit &fit, double quat[4], double *scale, double *angleDeg) {
	sift3d_affine_fit f;
	memset(&f, 0, sizeof(f));
	memcpy(f.A, fit.A, sizeof(f.A));
	f.status = fit.status;
	double s = 0, a = 0;
	const int rc = sift3d_fit_rotation(&f, 1, quat, &s, &a);
	if (rc != SIFT3D_OK) fprintf(stderr, "[3dsift_amd] FitRotation: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
	if (scale) *scale = s;
	if (angleDeg) *angleDeg = a;
	return rc == SIFT3D_OK && fit.status == 0;
}

namespace {
std::vector<Cvec> predict(const AffineFit *fits, size_t nfits, const std::vector<Keypoint> &kp) {
	const size_t n = kp.size();
	std::vector<Cvec> out(n, Cvec(NAN, NAN, NAN));
	if (nfits != 1 && nfits != n) {
		fprintf(stderr, "[3dsift_amd] PredictPositions: %zu fits for %zu keypoints (one fit, or one per keypoint)\n", nfits, n);
		return out;
	}
	std::vector<sift3d_affine_fit> f(nfits);
	for (size_t i = 0; i < nfits; i++) {
		memset(&f[i], 0, sizeof(f[i]));
		memcpy(f[i].A, fits[i].A, sizeof(f[i].A));
		f[i].status = fits[i].status;
	}
	std::vector<float> r(3 * (n ? n : 1)), p(3 * (n ? n : 1));
	for (size_t i = 0; i < n; i++) { r[3 * i] = kp[i].rx; r[3 * i + 1] = kp[i].ry; r[3 * i + 2] = kp[i].rz; }
	const int rc = sift3d_predict_positions(f.data(), (int)nfits, r.data(), (int)n, p.data());
	if (rc != SIFT3D_OK) {
		fprintf(stderr, "[3dsift_amd] PredictPositions: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
		return out;
	}
	for (size_t i = 0; i < n; i++) out[i] = Cvec(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
	return out;
}
}  // namespace

std::vector<Cvec> PredictPositions(const AffineFit &fit, const std::vector<Keypoint> &ref_kp) { return predict(&fit, 1, ref_kp); }
std::vector<Cvec> PredictPositions(const std::vector<AffineFit> &fits, const std::vector<Keypoint> &ref_kp) {
	return predict(fits.data(), fits.size(), ref_kp);
}

GuidedMatchResult GuidedMatch(std::vector<Cvec> &refMatch, std::vector<Cvec> &tarMatch, const std::vector<Keypoint> &ref_kp,
                              const std::vector<Keypoint> &tar_kp, const std::vector<Cvec> &predicted, float radius, double thresHold,
                              MatchMode mode) {
	GuidedMatchResult res;
	const size_t n = ref_kp.size(), m = tar_kp.size();
	if (predicted.size() != n) {
		fprintf(stderr, "[3dsift_amd] GuidedMatch: %zu predicted positions for %zu reference keypoints\n", predicted.size(), n);
		return res;
	}
	// gather the (possibly scattered) descriptor rows, as muBruteMatcher does; Keypoint::desc points into extractor-owned memory
	std::vector<float> a(n * SIFT3D_DESC_NUMEL), b(m * SIFT3D_DESC_NUMEL), ax(3 * (n ? n : 1)), bx(3 * (m ? m : 1)), px(3 * (n ? n : 1));
	for (size_t i = 0; i < n; i++) {
		if (ref_kp[i].desc) memcpy(&a[i * SIFT3D_DESC_NUMEL], ref_kp[i].desc, sizeof(float) * SIFT3D_DESC_NUMEL);
		ax[3 * i] = ref_kp[i].rx; ax[3 * i + 1] = ref_kp[i].ry; ax[3 * i + 2] = ref_kp[i].rz;
		px[3 * i] = predicted[i].x; px[3 * i + 1] = predicted[i].y; px[3 * i + 2] = predicted[i].z;
	}
	for (size_t j = 0; j < m; j++) {
		if (tar_kp[j].desc) memcpy(&b[j * SIFT3D_DESC_NUMEL], tar_kp[j].desc, sizeof(float) * SIFT3D_DESC_NUMEL);
		bx[3 * j] = tar_kp[j].rx; bx[3 * j + 1] = tar_kp[j].ry; bx[3 * j + 2] = tar_kp[j].rz;
	}
	std::vector<int> gi(n ? n : 1), si(n ? n : 1), cand(n ? n : 1);
	std::vector<float> gd(n ? n : 1), sd(n ? n : 1), pairs(6 * (n ? n : 1));
	int np = 0;
	const int rc = sift3d_match_guided(a.data(), ax.data(), (int)n, b.data(), bx.data(), (int)m, px.data(), radius, thresHold, (int)mode, 0,
	                                   GetDevice(), gi.data(), si.data(), gd.data(), sd.data(), cand.data(), pairs.data(), &np, &res.seconds);
	if (rc != SIFT3D_OK) {
		fprintf(stderr, "[3dsift_amd] GuidedMatch: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
		return res;
	}
	for (int i = 0; i < np; i++) {
		refMatch.push_back(Cvec(pairs[6 * i], pairs[6 * i + 1], pairs[6 * i + 2]));
		tarMatch.push_back(Cvec(pairs[6 * i + 3], pairs[6 * i + 4], pairs[6 * i + 5]));
	}
	res.glodenIdx.assign(gi.begin(), gi.begin() + n); res.silverIdx.assign(si.begin(), si.begin() + n);
	res.candidates.assign(cand.begin(), cand.begin() + n);
	res.glodenDistSquare.assign(gd.begin(), gd.begin() + n); res.silverDistSquare.assign(sd.begin(), sd.begin() + n);
	res.ok = true;
	return res;
}

Cvec IcgnResult::Displacement() const { return Cvec((float)p[0], (float)p[4], (float)p[8]); }
void IcgnResult::Gradient(double G[9]) const {
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 3; j++) G[3 * i + j] = p[4 * i + 1 + j];
}

bool PrefilterBSpline(const float *vol, int nx, int ny, int nz, float *coefficients, double *seconds) {
	const int rc = sift3d_bspline_prefilter(vol, nx, ny, nz, coefficients, 0, GetDevice(), seconds);
	if (rc != SIFT3D_OK) fprintf(stderr, "[3dsift_amd] PrefilterBSpline: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
	return rc == SIFT3D_OK;
}

bool UploadVolume(const void *vol, VoxelType type, int nx, int ny, int nz, float *d_dst, double *seconds) {
	const int rc = sift3d_volume_to_device(vol, (int)type, nx, ny, nz, 0, GetDevice(), d_dst, seconds);
	if (rc != SIFT3D_OK) fprintf(stderr, "[3dsift_amd] UploadVolume: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
	return rc == SIFT3D_OK;
}

Cvec SearchResult::Displacement() const { return Cvec((float)d[0], (float)d[1], (float)d[2]); }

std::vector<SearchResult> SearchDisplacements(const float *ref, int nx, int ny, int nz, const float *tar, int tnx, int tny, int tnz,
                                              const std::vector<Cvec> &points, const std::vector<Cvec> *guesses, const SearchOptions &opts) {
	const size_t m = points.size();
	std::vector<SearchResult> res(m);
	std::vector<int> q, g;
	if (!int_triples("SearchDisplacements", "point", points, q)) return res;
	if (guesses && guesses->size() != m) {
		fprintf(stderr, "[3dsift_amd] SearchDisplacements: %zu guesses for %zu points\n", guesses->size(), m);
		return res;
	}
	if (guesses && !int_triples("SearchDisplacements", "guess", *guesses, g)) return res;
	sift3d_search_options o;
	sift3d_default_search_options(&o);
	o.subset_radius = opts.subset_radius;
	o.search_radius = opts.search_radius;
	std::vector<sift3d_search_result> r(m ? m : 1);
	double sec = 0;
	const int rc = sift3d_zncc_search(ref, nx, ny, nz, tar, tnx, tny, tnz, q.data(), (int)m, guesses ? g.data() : nullptr, &o, 0, GetDevice(), r.data(),
	                                  &sec);
	if (rc != SIFT3D_OK) {
		fprintf(stderr, "[3dsift_amd] SearchDisplacements: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
		return res;
	}
	for (size_t i = 0; i < m; i++) {
		memcpy(res[i].d, r[i].d, sizeof(res[i].d));
		res[i].status = r[i].status;
		res[i].zncc = r[i].zncc;
		res[i].zncc_second = r[i].zncc_second;
		res[i].candidates = r[i].candidates;
		res[i].seconds = sec;
	}
	return res;
}

std::vector<SubsetQuality> SelectSubsets(const float *ref, int nx, int ny, int nz, const std::vector<Cvec> &points, const SubsetOptions &opts) {
	const size_t m = points.size();
	std::vector<SubsetQuality> res(m);
	std::vector<int> q;
	if (!int_triples("SelectSubsets", "point", points, q)) return res;
	sift3d_subset_options o;
	sift3d_default_subset_options(&o);
	o.r_min = opts.r_min;
	o.r_max = opts.r_max;
	o.criterion = opts.criterion;
	o.threshold = opts.threshold;
	o.level = opts.level;
	o.fraction_min = opts.fraction_min;
	std::vector<sift3d_subset_result> r(m ? m : 1);
	double sec = 0;
	const int rc = sift3d_subset_quality(ref, nx, ny, nz, q.data(), (int)m, &o, 0, GetDevice(), r.data(), &sec);
	if (rc != SIFT3D_OK) {
		fprintf(stderr, "[3dsift_amd] SelectSubsets: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
		return res;
	}
	for (size_t i = 0; i < m; i++) {
		res[i].mean = r[i].mean;
		res[i].dR = r[i].dR;
		memcpy(res[i].G, r[i].G, sizeof(res[i].G));
		memcpy(res[i].eig, r[i].eig, sizeof(res[i].eig));
		res[i].radius = r[i].radius;
		res[i].status = r[i].status;
		res[i].feasible = r[i].feasible;
		res[i].material = r[i].material;
		res[i].seconds = sec;
	}
	return res;
}

bool GroupSubsetsByRadius(const std::vector<SubsetQuality> &quality, int r_min, int r_max, std::vector<std::vector<int>> &groups) {
	const size_t m = quality.size();
	groups.clear();
	std::vector<sift3d_subset_result> r(m ? m : 1);
	memset(r.data(), 0, sizeof(sift3d_subset_result) * r.size());
	for (size_t i = 0; i < m; i++) {
		r[i].radius = quality[i].radius;
		r[i].status = quality[i].status;
	}
	std::vector<int> order(m ? m : 1), offsets(64, 0);  // the library takes at most 31 groups
	int count = 0;
	const int rc = sift3d_subset_group_by_radius(r.data(), (int)m, r_min, r_max, order.data(), offsets.data(), &count);
	if (rc != SIFT3D_OK) {
		fprintf(stderr, "[3dsift_amd] GroupSubsetsByRadius: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
		return false;
	}
	groups.resize(r_max - r_min + 1);
	for (int g = 0; g <= r_max - r_min; g++) groups[g].assign(order.begin() + offsets[g], order.begin() + offsets[g + 1]);
	return true;
}

// what RefineDisplacements and RefineDisplacementsMasked share: the initial parameters of the fits (a failed fit: a NaN row, or, with
// fallback, the search's displacement), the options record (without the interpolation, which the two calls map differently) and the
// conversion of the result records
static void icgn_init_rows(const std::vector<AffineFit> &init, const std::vector<SearchResult> *fallback, const std::vector<int> &q, size_t m,
                           std::vector<double> &p0) {
	std::vector<sift3d_affine_fit> f(m ? m : 1);
	memset(f.data(), 0, sizeof(sift3d_affine_fit) * f.size());
	for (size_t i = 0; i < m; i++) {
		memcpy(f[i].A, init[i].A, sizeof(f[i].A));
		f[i].status = init[i].status;
	}
	p0.assign(12 * (m ? m : 1), 0.0);
	sift3d_icgn_init_from_fits(f.data(), q.data(), (int)m, p0.data());
	if (fallback) {  // the NaN rows of the failed fits take the search's displacement
		std::vector<sift3d_search_result> sr(m ? m : 1);
		memset(sr.data(), 0, sizeof(sift3d_search_result) * sr.size());
		for (size_t i = 0; i < m; i++) {
			memcpy(sr[i].d, (*fallback)[i].d, sizeof(sr[i].d));
			sr[i].status = (*fallback)[i].status;
		}
		sift3d_icgn_init_from_search(sr.data(), (int)m, 1, p0.data());
	}
}

static sift3d_icgn_options icgn_options_of(const IcgnOptions &opts) {
	sift3d_icgn_options o;
	sift3d_default_icgn_options(&o);
	o.subset_radius = opts.subset_radius;
	o.max_iterations = opts.max_iterations;
	o.tolerance = opts.tolerance;
	return o;
}

static void icgn_records(const std::vector<sift3d_icgn_result> &r, double sec, std::vector<IcgnResult> &res) {
	for (size_t i = 0; i < res.size(); i++) {
		memcpy(res[i].p, r[i].p, sizeof(res[i].p));
		res[i].zncc = r[i].zncc;
		res[i].last_step = r[i].last_step;
		res[i].iterations = r[i].iterations;
		res[i].status = r[i].status;
		res[i].seconds = sec;
	}
}

std::vector<IcgnResult> RefineDisplacements(const float *ref, int nx, int ny, int nz, const float *tar, int tnx, int tny, int tnz,
                                            const std::vector<Cvec> &points, const std::vector<AffineFit> *init, const IcgnOptions &opts,
                                            const std::vector<SearchResult> *fallback) {
	return RefineDisplacements(ref, nx, ny, nz, tar, tnx, tny, tnz, points, init, opts, fallback, false);
}

std::vector<IcgnResult> RefineDisplacements(const float *ref, int nx, int ny, int nz, const float *tar, int tnx, int tny, int tnz,
                                            const std::vector<Cvec> &points, const std::vector<AffineFit> *init, const IcgnOptions &opts,
                                            const std::vector<SearchResult> *fallback, bool tar_is_coefficients) {
	const size_t m = points.size();
	std::vector<IcgnResult> res(m);
	std::vector<int> q;
	if (!int_triples("RefineDisplacements", "point", points, q)) return res;
	if (init && init->size() != m) {
		fprintf(stderr, "[3dsift_amd] RefineDisplacements: %zu initial fits for %zu points\n", init->size(), m);
		return res;
	}
	if (fallback && fallback->size() != m) {
		fprintf(stderr, "[3dsift_amd] RefineDisplacements: %zu fallback results for %zu points\n", fallback->size(), m);
		return res;
	}
	std::vector<double> p0;
	if (init) icgn_init_rows(*init, fallback, q, m, p0);
	sift3d_icgn_options o = icgn_options_of(opts);
	const bool bspline = opts.interpolation == 2;  // the C entry of its own: sift3d_icgn's option stays 0 / 1
	o.interpolation = bspline ? 0 : opts.interpolation;
	std::vector<sift3d_icgn_result> r(m ? m : 1);
	double sec = 0;
	const double *p0p = init ? p0.data() : nullptr;
	const int rc = bspline ? sift3d_icgn_bspline(ref, nx, ny, nz, tar, tnx, tny, tnz, q.data(), (int)m, p0p, &o, tar_is_coefficients ? 1 : 0, 0,
	                                             GetDevice(), r.data(), &sec)
	                       : sift3d_icgn(ref, nx, ny, nz, tar, tnx, tny, tnz, q.data(), (int)m, p0p, &o, 0, GetDevice(), r.data(), &sec);
	if (rc != SIFT3D_OK) {
		fprintf(stderr, "[3dsift_amd] RefineDisplacements: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
		return res;
	}
	icgn_records(r, sec, res);
	return res;
}

bool MaskFromLevel(const float *vol, int nx, int ny, int nz, double level, unsigned char *mask, double *seconds) {
	const int rc = sift3d_mask_from_level(vol, nx, ny, nz, level, mask, 0, GetDevice(), seconds);
	if (rc != SIFT3D_OK) fprintf(stderr, "[3dsift_amd] MaskFromLevel: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
	return rc == SIFT3D_OK;
}

std::vector<IcgnResult> RefineDisplacementsMasked(const float *ref, int nx, int ny, int nz, const float *tar, int tnx, int tny, int tnz,
                                                  const unsigned char *mask, const std::vector<Cvec> &points, const std::vector<AffineFit> *init,
                                                  const IcgnOptions &opts, float min_fraction, std::vector<int> *active,
                                                  bool tar_is_coefficients) {
	const size_t m = points.size();
	std::vector<IcgnResult> res(m);
	if (active) active->assign(m, 0);
	std::vector<int> q;
	if (!int_triples("RefineDisplacementsMasked", "point", points, q)) return res;
	if (init && init->size() != m) {
		fprintf(stderr, "[3dsift_amd] RefineDisplacementsMasked: %zu initial fits for %zu points\n", init->size(), m);
		return res;
	}
	std::vector<double> p0;
	if (init) icgn_init_rows(*init, nullptr, q, m, p0);
	sift3d_icgn_options o = icgn_options_of(opts);
	o.interpolation = opts.interpolation;  // 0, 1 or 2: one C entry for the three
	std::vector<sift3d_icgn_result> r(m ? m : 1);
	std::vector<int> n(m ? m : 1, 0);
	double sec = 0;
	const int rc = sift3d_icgn_masked(ref, nx, ny, nz, tar, tnx, tny, tnz, mask, q.data(), (int)m, init ? p0.data() : nullptr, &o, min_fraction,
	                                  tar_is_coefficients ? 1 : 0, 0, GetDevice(), r.data(), n.data(), &sec);
	if (rc != SIFT3D_OK) {
		fprintf(stderr, "[3dsift_amd] RefineDisplacementsMasked: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
		return res;
	}
	icgn_records(r, sec, res);
	if (active) active->assign(n.begin(), n.begin() + m);
	return res;
}

// true when labels is null (no labels) or holds one label per item; a message on stderr otherwise
static bool labels_fit(const char *who, const char *what, const std::vector<int> *labels, size_t m) {
	if (!labels || labels->size() == m) return true;
	fprintf(stderr, "[3dsift_amd] %s: %zu labels for %zu %s\n", who, labels->size(), m, what);
	return false;
}
// the pointer the C entry takes: never null, also for no items
static const int *label_data(const std::vector<int> &labels) {
	static const int none = 0;
	return labels.empty() ? &none : labels.data();
}

bool LabelMask(const unsigned char *mask, int nx, int ny, int nz, int connectivity, int min_voxels, int *labels, int *count, double *seconds) {
	const int rc = sift3d_mask_label(mask, nx, ny, nz, connectivity, min_voxels, labels, count, 0, GetDevice(), seconds);
	if (rc != SIFT3D_OK) fprintf(stderr, "[3dsift_amd] LabelMask: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
	return rc == SIFT3D_OK;
}

std::vector<int> LabelsAt(const int *labels, int nx, int ny, int nz, const std::vector<Cvec> &points) {
	const size_t m = points.size();
	std::vector<int> q, out(m ? m : 1, 0);
	if (!int_triples("LabelsAt", "point", points, q)) return std::vector<int>();
	const int rc = sift3d_labels_at_points(labels, nx, ny, nz, q.data(), (int)m, out.data(), 0, GetDevice());
	if (rc != SIFT3D_OK) {
		fprintf(stderr, "[3dsift_amd] LabelsAt: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
		return std::vector<int>();
	}
	out.resize(m);
	return out;
}

bool DistanceTransform(const unsigned char *mask, int nx, int ny, int nz, bool border, int *dist2, double *seconds) {
	const int rc = sift3d_mask_distance(mask, nx, ny, nz, border ? 1 : 0, dist2, 0, GetDevice(), seconds);
	if (rc != SIFT3D_OK) fprintf(stderr, "[3dsift_amd] DistanceTransform: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
	return rc == SIFT3D_OK;
}

bool ErodeMask(const int *dist2, int nx, int ny, int nz, int level2, unsigned char *mask, double *seconds) {
	const int rc = sift3d_mask_from_distance(dist2, nx, ny, nz, level2, mask, 0, GetDevice(), seconds);
	if (rc != SIFT3D_OK) fprintf(stderr, "[3dsift_amd] ErodeMask: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
	return rc == SIFT3D_OK;
}

std::vector<int> DistancesAt(const int *dist2, int nx, int ny, int nz, const std::vector<Cvec> &points) {
	const size_t m = points.size();
	std::vector<int> q, out(m ? m : 1, 0);
	if (!int_triples("DistancesAt", "point", points, q)) return std::vector<int>();
	const int rc = sift3d_distance_at_points(dist2, nx, ny, nz, q.data(), (int)m, out.data(), 0, GetDevice());
	if (rc != SIFT3D_OK) {
		fprintf(stderr, "[3dsift_amd] DistancesAt: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
		return std::vector<int>();
	}
	out.resize(m);
	return out;
}

bool SplitBodies(const unsigned char *mask, int nx, int ny, int nz, int *labels, int *count, const SplitOptions &o, int *dist2, SplitInfo *info,
                 double *seconds) {
	sift3d_split_options c;
	sift3d_default_split_options(&c);
	c.connectivity = o.connectivity;
	c.core_dist2 = o.core_dist2;
	c.min_core_voxels = o.min_core_voxels;
	c.border = o.border ? 1 : 0;
	c.max_rounds = o.max_rounds;
	c.keep_unreached = o.keep_unreached ? 1 : 0;
	c.min_voxels = o.min_voxels;
	sift3d_split_info i = {0, 0, 0, 0};
	const int rc = sift3d_mask_split(mask, nx, ny, nz, &c, labels, count, dist2, &i, 0, GetDevice(), seconds);
	if (rc != SIFT3D_OK) fprintf(stderr, "[3dsift_amd] SplitBodies: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
	if (info && rc == SIFT3D_OK) {
		info->cores = i.cores;
		info->unreached_bodies = i.unreached_bodies;
		info->rounds = i.rounds;
		info->unlabelled = i.unlabelled;
	}
	return rc == SIFT3D_OK;
}

std::vector<AffineFit> EstimateBodyRigid(const std::vector<Cvec> &ref, const std::vector<Cvec> &tar, const int *labels, int nx, int ny, int nz,
                                         int count, FitModel model, const RansacOptions &opts, std::vector<int> *pairLabels,
                                         std::vector<int> *inlierMask) {
	const size_t n = ref.size() < tar.size() ? ref.size() : tar.size();
	if (pairLabels) pairLabels->assign(n, 0);
	if (inlierMask) inlierMask->assign(n, 0);
	const std::vector<float> p = pairs6(ref, tar, n);
	std::vector<int> lab(n ? n : 1, 0);
	int rc = sift3d_labels_at_positions(labels, nx, ny, nz, p.data(), 6, (int)n, lab.data(), 0, GetDevice());
	const sift3d_ransac_options o = to_c(opts);
	std::vector<sift3d_affine_fit> f(count > 0 ? count : 1);
	std::vector<unsigned char> mask(n ? n : 1);
	double sec = 0;
	if (rc == SIFT3D_OK) rc = sift3d_fit_rigid_bodies(p.data(), (int)n, lab.data(), count, (int)model, &o, 0, GetDevice(), f.data(), mask.data(), &sec);
	if (rc != SIFT3D_OK) {
		fprintf(stderr, "[3dsift_amd] EstimateBodyRigid: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
		return std::vector<AffineFit>();
	}
	std::vector<AffineFit> res(count);
	for (int b = 0; b < count; b++) from_c(f[b], sec, res[b]);
	if (pairLabels) pairLabels->assign(lab.begin(), lab.begin() + n);
	if (inlierMask) inlierMask->assign(mask.begin(), mask.begin() + n);
	return res;
}

std::vector<AffineFit> SeedsFromBodyFits(const std::vector<AffineFit> &fits, const std::vector<int> &pointLabels) {
	std::vector<AffineFit> res(pointLabels.size());
	for (size_t i = 0; i < res.size(); i++) {
		const int L = pointLabels[i];
		if (L >= 1 && (size_t)L <= fits.size()) res[i] = fits[L - 1];
		else res[i].status = 1;
	}
	return res;
}

std::vector<IcgnResult> RefineDisplacementsLabelled(const float *ref, int nx, int ny, int nz, const float *tar, int tnx, int tny, int tnz,
                                                    const int *labels, const std::vector<Cvec> &points, const std::vector<AffineFit> *init,
                                                    const IcgnOptions &opts, float min_fraction, std::vector<int> *active,
                                                    std::vector<int> *pointLabels, bool tar_is_coefficients) {
	const size_t m = points.size();
	std::vector<IcgnResult> res(m);
	if (active) active->assign(m, 0);
	if (pointLabels) pointLabels->assign(m, 0);
	std::vector<int> q;
	if (!int_triples("RefineDisplacementsLabelled", "point", points, q)) return res;
	if (init && init->size() != m) {
		fprintf(stderr, "[3dsift_amd] RefineDisplacementsLabelled: %zu initial fits for %zu points\n", init->size(), m);
		return res;
	}
	std::vector<double> p0;
	if (init) icgn_init_rows(*init, nullptr, q, m, p0);
	sift3d_icgn_options o = icgn_options_of(opts);
	o.interpolation = opts.interpolation;  // 0, 1 or 2: one C entry for the three
	std::vector<sift3d_icgn_result> r(m ? m : 1);
	std::vector<int> n(m ? m : 1, 0), lab(m ? m : 1, 0);
	double sec = 0;
	const int rc = sift3d_icgn_labelled(ref, nx, ny, nz, tar, tnx, tny, tnz, labels, q.data(), (int)m, init ? p0.data() : nullptr, &o, min_fraction,
	                                    tar_is_coefficients ? 1 : 0, 0, GetDevice(), r.data(), n.data(), lab.data(), &sec);
	if (rc != SIFT3D_OK) {
		fprintf(stderr, "[3dsift_amd] RefineDisplacementsLabelled: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
		return res;
	}
	icgn_records(r, sec, res);
	if (active) active->assign(n.begin(), n.begin() + m);
	if (pointLabels) pointLabels->assign(lab.begin(), lab.begin() + m);
	return res;
}

// the strain call behind the ComputeStrains overloads: rc is what the input conversion returned; labels null: the unlabelled call
static std::vector<StrainResult> strains_of(const std::vector<int> &q, size_t m, int rc, const std::vector<double> &u,
                                            const std::vector<unsigned char> &valid, const StrainOptions &opts,
                                            const std::vector<int> *labels = nullptr) {
	std::vector<StrainResult> res(m);
	if (!labels_fit("ComputeStrains", "points", labels, m)) return res;
	sift3d_strain_options o;
	sift3d_default_strain_options(&o);
	o.radius = opts.radius;
	o.min_neighbours = opts.min_neighbours;
	o.measure = opts.measure;
	std::vector<sift3d_strain_result> r(m ? m : 1);
	double sec = 0;
	if (rc == SIFT3D_OK && labels)
		rc = sift3d_strain_labelled(q.data(), u.data(), valid.data(), label_data(*labels), (int)m, &o, 0, GetDevice(), r.data(), &sec);
	else if (rc == SIFT3D_OK)
		rc = sift3d_strain(q.data(), u.data(), valid.data(), (int)m, &o, 0, GetDevice(), r.data(), &sec);
	if (rc != SIFT3D_OK) {
		fprintf(stderr, "[3dsift_amd] ComputeStrains: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
		return res;
	}
	for (size_t i = 0; i < m; i++) {
		memcpy(res[i].disp, r[i].disp, sizeof(res[i].disp));
		memcpy(res[i].G, r[i].G, sizeof(res[i].G));
		memcpy(res[i].E, r[i].E, sizeof(res[i].E));
		memcpy(res[i].principal, r[i].principal, sizeof(res[i].principal));
		res[i].equivalent = r[i].equivalent;
		res[i].rms = r[i].rms;
		res[i].neighbours = r[i].neighbours;
		res[i].status = r[i].status;
		res[i].seconds = sec;
	}
	return res;
}

// the C records of m shell results (p, zncc, status; the rest zero)
template <class CRecord, class Result>
static std::vector<CRecord> c_records(const std::vector<Result> &disp, size_t m) {
	std::vector<CRecord> ic(m ? m : 1);
	memset(ic.data(), 0, sizeof(CRecord) * ic.size());
	for (size_t i = 0; i < m; i++) {
		memcpy(ic[i].p, disp[i].p, sizeof(ic[i].p));
		ic[i].zncc = disp[i].zncc;
		ic[i].status = disp[i].status;
	}
	return ic;
}

// valid[i] stays set only where keep[i] is (keep null: as it is); false (message on stderr) when keep has the wrong length
static bool apply_keep(const std::vector<unsigned char> *keep, size_t m, std::vector<unsigned char> &valid) {
	if (!keep) return true;
	if (keep->size() != m) {
		fprintf(stderr, "[3dsift_amd] ComputeStrains: %zu keep bytes for %zu points\n", keep->size(), m);
		return false;
	}
	for (size_t i = 0; i < m; i++) valid[i] = valid[i] && (*keep)[i] ? 1 : 0;
	return true;
}

static std::vector<StrainResult> strains_first(const std::vector<Cvec> &points, const std::vector<IcgnResult> &disp,
                                               const std::vector<unsigned char> *keep, const StrainOptions &opts, double zncc_min,
                                               bool accept_unconverged, const std::vector<int> *labels = nullptr) {
	const size_t m = points.size();
	std::vector<StrainResult> res(m);
	std::vector<int> q;
	if (!int_triples("ComputeStrains", "point", points, q)) return res;
	if (disp.size() != m) {
		fprintf(stderr, "[3dsift_amd] ComputeStrains: %zu displacements for %zu points\n", disp.size(), m);
		return res;
	}
	const std::vector<sift3d_icgn_result> ic = c_records<sift3d_icgn_result>(disp, m);
	std::vector<double> u(3 * (m ? m : 1));
	std::vector<unsigned char> valid(m ? m : 1);
	const int rc = sift3d_strain_input_from_icgn(ic.data(), (int)m, zncc_min, accept_unconverged ? 1 : 0, u.data(), valid.data());
	if (!apply_keep(keep, m, valid)) return res;
	return strains_of(q, m, rc, u, valid, opts, labels);
}

std::vector<StrainResult> ComputeStrains(const std::vector<Cvec> &points, const std::vector<IcgnResult> &disp, const StrainOptions &opts, double zncc_min,
                                         bool accept_unconverged) {
	return strains_first(points, disp, nullptr, opts, zncc_min, accept_unconverged);
}
std::vector<StrainResult> ComputeStrains(const std::vector<Cvec> &points, const std::vector<IcgnResult> &disp, const std::vector<unsigned char> &keep,
                                         const StrainOptions &opts, double zncc_min, bool accept_unconverged) {
	return strains_first(points, disp, &keep, opts, zncc_min, accept_unconverged);
}
std::vector<StrainResult> ComputeStrains(const std::vector<Cvec> &points, const std::vector<IcgnResult> &disp, const std::vector<int> &labels,
                                         const std::vector<unsigned char> *keep, const StrainOptions &opts, double zncc_min,
                                         bool accept_unconverged) {
	return strains_first(points, disp, keep, opts, zncc_min, accept_unconverged, &labels);
}

Cvec Icgn2Result::Displacement() const { return Cvec((float)p[0], (float)p[10], (float)p[20]); }
void Icgn2Result::Gradient(double G[9]) const {
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 3; j++) G[3 * i + j] = p[10 * i + 1 + j];
}
void Icgn2Result::SecondDerivatives(double S[18]) const {
	for (int i = 0; i < 3; i++)
		for (int j = 0; j < 6; j++) S[6 * i + j] = p[10 * i + 4 + j];
}

std::vector<Icgn2Result> RefineDisplacementsSecondOrder(const float *ref, int nx, int ny, int nz, const float *tar, int tnx, int tny, int tnz,
                                                        const std::vector<Cvec> &points, const std::vector<IcgnResult> &first,
                                                        const IcgnOptions &opts, bool tar_is_coefficients) {
	const size_t m = points.size();
	std::vector<Icgn2Result> res(m);
	std::vector<int> q;
	if (!int_triples("RefineDisplacementsSecondOrder", "point", points, q)) return res;
	if (first.size() != m) {
		fprintf(stderr, "[3dsift_amd] RefineDisplacementsSecondOrder: %zu first-order results for %zu points\n", first.size(), m);
		return res;
	}
	std::vector<sift3d_icgn_result> f(m ? m : 1);
	memset(f.data(), 0, sizeof(sift3d_icgn_result) * f.size());
	for (size_t i = 0; i < m; i++) {
		memcpy(f[i].p, first[i].p, sizeof(f[i].p));
		f[i].status = first[i].status;
	}
	std::vector<double> p0(30 * (m ? m : 1), 0.0);
	sift3d_icgn2_init_from_icgn(f.data(), (int)m, p0.data());
	sift3d_icgn_options o;
	sift3d_default_icgn_options(&o);
	o.subset_radius = opts.subset_radius;
	o.max_iterations = opts.max_iterations;
	o.tolerance = opts.tolerance;
	o.interpolation = opts.interpolation;
	std::vector<sift3d_icgn2_result> r(m ? m : 1);
	double sec = 0;
	const int rc = sift3d_icgn2(ref, nx, ny, nz, tar, tnx, tny, tnz, q.data(), (int)m, p0.data(), &o, tar_is_coefficients ? 1 : 0, 0, GetDevice(),
	                            r.data(), &sec);
	if (rc != SIFT3D_OK) {
		fprintf(stderr, "[3dsift_amd] RefineDisplacementsSecondOrder: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
		return res;
	}
	for (size_t i = 0; i < m; i++) {
		memcpy(res[i].p, r[i].p, sizeof(res[i].p));
		res[i].zncc = r[i].zncc;
		res[i].last_step = r[i].last_step;
		res[i].iterations = r[i].iterations;
		res[i].status = r[i].status;
		res[i].seconds = sec;
	}
	return res;
}

static std::vector<StrainResult> strains_second(const std::vector<Cvec> &points, const std::vector<Icgn2Result> &disp,
                                                const std::vector<unsigned char> *keep, const StrainOptions &opts, double zncc_min,
                                                bool accept_unconverged, const std::vector<int> *labels = nullptr) {
	const size_t m = points.size();
	std::vector<int> q;
	if (!int_triples("ComputeStrains", "point", points, q)) return std::vector<StrainResult>(m);
	if (disp.size() != m) {
		fprintf(stderr, "[3dsift_amd] ComputeStrains: %zu displacements for %zu points\n", disp.size(), m);
		return std::vector<StrainResult>(m);
	}
	const std::vector<sift3d_icgn2_result> ic = c_records<sift3d_icgn2_result>(disp, m);
	std::vector<double> u(3 * (m ? m : 1));
	std::vector<unsigned char> valid(m ? m : 1);
	const int rc = sift3d_strain_input_from_icgn2(ic.data(), (int)m, zncc_min, accept_unconverged ? 1 : 0, u.data(), valid.data());
	if (!apply_keep(keep, m, valid)) return std::vector<StrainResult>(m);
	return strains_of(q, m, rc, u, valid, opts, labels);
}

std::vector<StrainResult> ComputeStrains(const std::vector<Cvec> &points, const std::vector<Icgn2Result> &disp, const StrainOptions &opts,
                                         double zncc_min, bool accept_unconverged) {
	return strains_second(points, disp, nullptr, opts, zncc_min, accept_unconverged);
}
std::vector<StrainResult> ComputeStrains(const std::vector<Cvec> &points, const std::vector<Icgn2Result> &disp, const std::vector<unsigned char> &keep,
                                         const StrainOptions &opts, double zncc_min, bool accept_unconverged) {
	return strains_second(points, disp, &keep, opts, zncc_min, accept_unconverged);
}
std::vector<StrainResult> ComputeStrains(const std::vector<Cvec> &points, const std::vector<Icgn2Result> &disp, const std::vector<int> &labels,
                                         const std::vector<unsigned char> *keep, const StrainOptions &opts, double zncc_min,
                                         bool accept_unconverged) {
	return strains_second(points, disp, keep, opts, zncc_min, accept_unconverged, &labels);
}

// the validation call behind the ValidateDisplacements overloads: rc is what the input conversion returned; labels null: the unlabelled call
static std::vector<ValidationResult> validation_of(const std::vector<int> &q, size_t m, int rc, const std::vector<double> &u,
                                                   const std::vector<double> &g, bool use_gradients, const std::vector<unsigned char> &valid,
                                                   const ValidationOptions &opts, const std::vector<int> *labels) {
	std::vector<ValidationResult> res(m);
	if (!labels_fit("ValidateDisplacements", "points", labels, m)) return res;
	sift3d_validate_options o;
	sift3d_default_validate_options(&o);
	o.radius = opts.radius;
	o.min_neighbours = opts.min_neighbours;
	o.passes = opts.passes;
	o.threshold = opts.threshold;
	o.eps = opts.eps;
	std::vector<sift3d_validate_result> r(m ? m : 1);
	double sec = 0;
	if (rc == SIFT3D_OK && labels)
		rc = sift3d_validate_displacements_labelled(q.data(), u.data(), use_gradients ? g.data() : nullptr, valid.data(), label_data(*labels), (int)m,
		                                            &o, 0, GetDevice(), r.data(), &sec);
	else if (rc == SIFT3D_OK)
		rc = sift3d_validate_displacements(q.data(), u.data(), use_gradients ? g.data() : nullptr, valid.data(), (int)m, &o, 0, GetDevice(), r.data(),
		                                   &sec);
	if (rc != SIFT3D_OK) {
		fprintf(stderr, "[3dsift_amd] ValidateDisplacements: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
		return res;
	}
	for (size_t i = 0; i < m; i++) {
		memcpy(res[i].median, r[i].median, sizeof(res[i].median));
		memcpy(res[i].mad, r[i].mad, sizeof(res[i].mad));
		res[i].score = r[i].score;
		res[i].neighbours = r[i].neighbours;
		res[i].status = r[i].status;
		res[i].flagged = r[i].flagged;
		res[i].pass = r[i].pass;
		res[i].seconds = sec;
	}
	return res;
}

template <class CRecord, class Result, class Convert>
static std::vector<ValidationResult> validate_results(const std::vector<Cvec> &points, const std::vector<Result> &disp, const ValidationOptions &opts,
                                                      double zncc_min, bool accept_unconverged, bool use_gradients, Convert convert,
                                                      const std::vector<int> *labels = nullptr) {
	const size_t m = points.size();
	std::vector<int> q;
	if (!int_triples("ValidateDisplacements", "point", points, q)) return std::vector<ValidationResult>(m);
	if (disp.size() != m) {
		fprintf(stderr, "[3dsift_amd] ValidateDisplacements: %zu displacements for %zu points\n", disp.size(), m);
		return std::vector<ValidationResult>(m);
	}
	const std::vector<CRecord> ic = c_records<CRecord>(disp, m);
	std::vector<double> u(3 * (m ? m : 1)), g(9 * (m ? m : 1));
	std::vector<unsigned char> valid(m ? m : 1);
	const int rc = convert(ic.data(), (int)m, zncc_min, accept_unconverged ? 1 : 0, u.data(), g.data(), valid.data());
	return validation_of(q, m, rc, u, g, use_gradients, valid, opts, labels);
}

std::vector<ValidationResult> ValidateDisplacements(const std::vector<Cvec> &points, const std::vector<IcgnResult> &disp, const ValidationOptions &opts,
                                                    double zncc_min, bool accept_unconverged, bool use_gradients) {
	return validate_results<sift3d_icgn_result>(points, disp, opts, zncc_min, accept_unconverged, use_gradients, sift3d_validate_input_from_icgn);
}
std::vector<ValidationResult> ValidateDisplacements(const std::vector<Cvec> &points, const std::vector<Icgn2Result> &disp, const ValidationOptions &opts,
                                                    double zncc_min, bool accept_unconverged, bool use_gradients) {
	return validate_results<sift3d_icgn2_result>(points, disp, opts, zncc_min, accept_unconverged, use_gradients, sift3d_validate_input_from_icgn2);
}
std::vector<ValidationResult> ValidateDisplacements(const std::vector<Cvec> &points, const std::vector<IcgnResult> &disp, const std::vector<int> &labels,
                                                    const ValidationOptions &opts, double zncc_min, bool accept_unconverged, bool use_gradients) {
	return validate_results<sift3d_icgn_result>(points, disp, opts, zncc_min, accept_unconverged, use_gradients, sift3d_validate_input_from_icgn,
	                                            &labels);
}
std::vector<ValidationResult> ValidateDisplacements(const std::vector<Cvec> &points, const std::vector<Icgn2Result> &disp, const std::vector<int> &labels,
                                                    const ValidationOptions &opts, double zncc_min, bool accept_unconverged, bool use_gradients) {
	return validate_results<sift3d_icgn2_result>(points, disp, opts, zncc_min, accept_unconverged, use_gradients, sift3d_validate_input_from_icgn2,
	                                             &labels);
}

// the C records of the shell's validation results
static std::vector<sift3d_validate_result> c_validation(const std::vector<ValidationResult> &v) {
	std::vector<sift3d_validate_result> r(v.size() ? v.size() : 1);
	memset(r.data(), 0, sizeof(sift3d_validate_result) * r.size());
	for (size_t i = 0; i < v.size(); i++) {
		memcpy(r[i].median, v[i].median, sizeof(r[i].median));
		memcpy(r[i].mad, v[i].mad, sizeof(r[i].mad));
		r[i].score = v[i].score;
		r[i].neighbours = v[i].neighbours;
		r[i].status = v[i].status;
		r[i].flagged = v[i].flagged;
		r[i].pass = v[i].pass;
	}
	return r;
}

std::vector<unsigned char> KeepMask(const std::vector<ValidationResult> &validation) {
	const size_t m = validation.size();
	std::vector<unsigned char> keep(m ? m : 1);
	sift3d_validate_keep(c_validation(validation).data(), nullptr, (int)m, keep.data());
	keep.resize(m);
	return keep;
}

std::vector<AffineFit> SeedsFromValidation(const std::vector<Cvec> &points, const std::vector<IcgnResult> &first,
                                           const std::vector<ValidationResult> &validation) {
	const size_t m = points.size();
	std::vector<AffineFit> seeds(m);
	for (size_t i = 0; i < m; i++) seeds[i].status = 1;
	if (first.size() != m || validation.size() != m) {
		fprintf(stderr, "[3dsift_amd] SeedsFromValidation: %zu results and %zu validation records for %zu points\n", first.size(), validation.size(), m);
		return seeds;
	}
	// the rows sift3d_icgn_init_from_validation writes are the reseeded points: every row starts as NaN and a written row is finite
	std::vector<double> p0(12 * (m ? m : 1), (double)NAN);
	sift3d_icgn_init_from_validation(c_validation(validation).data(), (int)m, p0.data(), nullptr);
	for (size_t i = 0; i < m; i++) {
		const double *p = p0.data() + 12 * i;
		const bool reseed = std::isfinite(p[0]) && std::isfinite(p[4]) && std::isfinite(p[8]);
		const bool kept = validation[i].status == 0 && !validation[i].flagged;
		if (!reseed && !kept) continue;
		const double q[3] = {points[i].x, points[i].y, points[i].z};
		for (int c = 0; c < 3; c++) {
			double L[3], u = reseed ? p[4 * c] : first[i].p[4 * c];
			for (int a = 0; a < 3; a++) L[a] = (a == c ? 1.0 : 0.0) + (reseed ? 0.0 : first[i].p[4 * c + 1 + a]);
			// b_c = q_c + u_c - L_c . q
			for (int a = 0; a < 3; a++) seeds[i].A[4 * c + a] = L[a];
			seeds[i].A[4 * c + 3] = (q[c] + u) - ((L[0] * q[0] + L[1] * q[1]) + L[2] * q[2]);
		}
		seeds[i].status = 0;
	}
	return seeds;
}

// the C records of shell field results (the seconds dropped)
static std::vector<sift3d_field_result> c_field(const std::vector<FieldResult> &f) {
	std::vector<sift3d_field_result> r(f.size() ? f.size() : 1);
	memset(r.data(), 0, sizeof(sift3d_field_result) * r.size());
	for (size_t i = 0; i < f.size(); i++) {
		memcpy(r[i].disp, f[i].disp, sizeof(r[i].disp));
		memcpy(r[i].G, f[i].G, sizeof(r[i].G));
		r[i].rms = f[i].rms;
		r[i].wsum = f[i].wsum;
		r[i].neighbours = f[i].neighbours;
		r[i].sides = f[i].sides;
		r[i].status = f[i].status;
	}
	return r;
}

// the call behind the EvaluateField overloads; labels and query_labels both null: the unlabelled call
static std::vector<FieldResult> field_of(const std::vector<Cvec> &points, const std::vector<IcgnResult> &disp, const std::vector<int> *labels,
                                         const std::vector<double> &queries3, const std::vector<int> *query_labels, const FieldOptions &opts,
                                         double zncc_min, bool accept_unconverged) {
	const size_t m = points.size(), nq = queries3.size() / 3;
	std::vector<FieldResult> res(nq);
	std::vector<int> q;
	if (!int_triples("EvaluateField", "point", points, q)) return res;
	if (!labels_fit("EvaluateField", "points", labels, m) || !labels_fit("EvaluateField", "queries", query_labels, nq)) return res;
	if (disp.size() != m || queries3.size() != 3 * nq) {
		fprintf(stderr, "[3dsift_amd] EvaluateField: %zu displacements for %zu points, %zu query coordinates\n", disp.size(), m, queries3.size());
		return res;
	}
	const std::vector<sift3d_icgn_result> ic = c_records<sift3d_icgn_result>(disp, m);
	std::vector<double> u(3 * (m ? m : 1));
	std::vector<unsigned char> valid(m ? m : 1);
	int rc = sift3d_strain_input_from_icgn(ic.data(), (int)m, zncc_min, accept_unconverged ? 1 : 0, u.data(), valid.data());
	sift3d_field_options o;
	sift3d_default_field_options(&o);
	o.radius = opts.radius;
	o.min_neighbours = opts.min_neighbours;
	o.weighting = opts.weighting;
	o.require_enclosed = opts.require_enclosed ? 1 : 0;
	std::vector<sift3d_field_result> r(nq ? nq : 1);
	double sec = 0;
	if (rc == SIFT3D_OK && labels)
		rc = sift3d_field_eval_labelled(q.data(), u.data(), valid.data(), label_data(*labels), (int)m, queries3.data(), label_data(*query_labels),
		                                (int)nq, &o, 0, GetDevice(), r.data(), &sec);
	else if (rc == SIFT3D_OK)
		rc = sift3d_field_eval(q.data(), u.data(), valid.data(), (int)m, queries3.data(), (int)nq, &o, 0, GetDevice(), r.data(), &sec);
	if (rc != SIFT3D_OK) {
		fprintf(stderr, "[3dsift_amd] EvaluateField: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
		return res;
	}
	for (size_t i = 0; i < nq; i++) {
		memcpy(res[i].disp, r[i].disp, sizeof(res[i].disp));
		memcpy(res[i].G, r[i].G, sizeof(res[i].G));
		res[i].rms = r[i].rms;
		res[i].wsum = r[i].wsum;
		res[i].neighbours = r[i].neighbours;
		res[i].sides = r[i].sides;
		res[i].status = r[i].status;
		res[i].seconds = sec;
	}
	return res;
}

std::vector<FieldResult> EvaluateField(const std::vector<Cvec> &points, const std::vector<IcgnResult> &disp, const std::vector<double> &queries3,
                                       const FieldOptions &opts, double zncc_min, bool accept_unconverged) {
	return field_of(points, disp, nullptr, queries3, nullptr, opts, zncc_min, accept_unconverged);
}
std::vector<FieldResult> EvaluateField(const std::vector<Cvec> &points, const std::vector<IcgnResult> &disp, const std::vector<int> &labels,
                                       const std::vector<double> &queries3, const std::vector<int> &query_labels, const FieldOptions &opts,
                                       double zncc_min, bool accept_unconverged) {
	return field_of(points, disp, &labels, queries3, &query_labels, opts, zncc_min, accept_unconverged);
}

std::vector<FieldResult> EvaluateField(const std::vector<Cvec> &points, const std::vector<IcgnResult> &disp, const std::vector<Cvec> &pointsA,
                                       const std::vector<IcgnResult> &stepA, const FieldOptions &opts, double zncc_min, bool accept_unconverged) {
	const size_t mA = pointsA.size();
	std::vector<int> qa;
	if (!int_triples("EvaluateField", "step A point", pointsA, qa)) return std::vector<FieldResult>(mA);
	if (stepA.size() != mA) {
		fprintf(stderr, "[3dsift_amd] EvaluateField: %zu step A results for %zu points\n", stepA.size(), mA);
		return std::vector<FieldResult>(mA);
	}
	std::vector<double> ua(3 * (mA ? mA : 1)), x(3 * mA);
	for (size_t i = 0; i < mA; i++)
		for (int c = 0; c < 3; c++) ua[3 * i + c] = stepA[i].p[4 * c];
	sift3d_field_queries_from_displacements(qa.data(), ua.data(), (int)mA, x.data());
	return EvaluateField(points, disp, x, opts, zncc_min, accept_unconverged);
}

std::vector<FieldResult> ComposeDisplacements(const std::vector<IcgnResult> &stepA, const std::vector<FieldResult> &atB) {
	const size_t m = stepA.size();
	std::vector<FieldResult> res(m);
	if (atB.size() != m) {
		fprintf(stderr, "[3dsift_amd] ComposeDisplacements: %zu field records for %zu results\n", atB.size(), m);
		return res;
	}
	std::vector<double> ua(3 * (m ? m : 1)), ga(9 * (m ? m : 1)), u(3 * (m ? m : 1)), g(9 * (m ? m : 1));
	std::vector<unsigned char> va(m ? m : 1), v(m ? m : 1);
	for (size_t i = 0; i < m; i++) {
		for (int c = 0; c < 3; c++) {
			ua[3 * i + c] = stepA[i].p[4 * c];
			for (int a = 0; a < 3; a++) ga[9 * i + 3 * c + a] = stepA[i].p[4 * c + 1 + a];
		}
		va[i] = stepA[i].status == 0 ? 1 : 0;
	}
	const int rc = sift3d_compose_displacements(ua.data(), ga.data(), va.data(), c_field(atB).data(), (int)m, u.data(), g.data(), v.data());
	if (rc != SIFT3D_OK) {
		fprintf(stderr, "[3dsift_amd] ComposeDisplacements: %s (%s)\n", sift3d_error_string(rc), sift3d_last_error());
		return res;
	}
	for (size_t i = 0; i < m; i++) {
		if (!v[i]) continue;
		memcpy(res[i].disp, u.data() + 3 * i, sizeof(res[i].disp));
		memcpy(res[i].G, g.data() + 9 * i, sizeof(res[i].G));
		res[i].rms = atB[i].rms;
		res[i].wsum = atB[i].wsum;
		res[i].neighbours = atB[i].neighbours;
		res[i].sides = atB[i].sides;
		res[i].status = 0;
	}
	return res;
}

std::vector<AffineFit> SeedsFromField(const std::vector<Cvec> &points, const std::vector<FieldResult> &field) {
	const size_t m = points.size();
	std::vector<AffineFit> seeds(m);
	for (size_t i = 0; i < m; i++) seeds[i].status = 1;
	if (field.size() != m) {
		fprintf(stderr, "[3dsift_amd] SeedsFromField: %zu field records for %zu points\n", field.size(), m);
		return seeds;
	}
	const std::vector<sift3d_field_result> rec = c_field(field);
	std::vector<double> u(3 * (m ? m : 1)), g(9 * (m ? m : 1)), p0(12 * (m ? m : 1), (double)NAN);
	std::vector<unsigned char> v(m ? m : 1);
	sift3d_field_unpack(rec.data(), (int)m, u.data(), g.data(), v.data());
	sift3d_icgn_init_from_field(u.data(), g.data(), v.data(), (int)m, 1, p0.data(), nullptr);
	for (size_t i = 0; i < m; i++) {
		if (!v[i]) continue;
		const double *p = p0.data() + 12 * i;
		const double q[3] = {points[i].x, points[i].y, points[i].z};
		for (int c = 0; c < 3; c++) {
			double L[3];
			for (int a = 0; a < 3; a++) L[a] = (a == c ? 1.0 : 0.0) + p[4 * c + 1 + a];
			// b_c = q_c + u_c - L_c . q
			for (int a = 0; a < 3; a++) seeds[i].A[4 * c + a] = L[a];
			seeds[i].A[4 * c + 3] = (q[c] + p[4 * c]) - ((L[0] * q[0] + L[1] * q[1]) + L[2] * q[2]);
		}
		seeds[i].status = 0;
	}
	return seeds;
}

}  // namespace CPUSIFT
