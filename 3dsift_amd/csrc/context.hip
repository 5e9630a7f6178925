// context.hip -- life cycle of a context, the KpSiftAlgorithm pipeline and its accessors (C-ABI: include/sift3d_hip.h).
//
// One sift3d_ctx (ctx_internal.h) owns a device arena (both pyramids, scratch, keypoint lists), a set of HIP streams and
// the host-built constant tables (tables.hip).  sift3d_run enqueues the whole KpSiftAlgorithm pipeline
// (reference Src/cSIFT3D.cc:165-235) on those streams with no host synchronisation inside; the
// only sync is the final one that also brings the keypoint count back.  r06: the other entry points live in entry_free.hip (the
// reference's free functions), entry_slab.hip (seeded / z-slab contexts) and entry_test.hip (hooks, debug entry points).
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <thread>

#include "ctx_internal.h"

#pragma clang fp contract(off)

namespace s3d {

static thread_local std::string g_last_error;
void set_last_error(const std::string &s) { g_last_error = s; }

int set_device(int device) {
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
		set_last_error("no HIP device visible: this library has no CPU fallback");
		return SIFT3D_ERR_NO_DEVICE;
	}
	if (device < 0 || device >= n) { set_last_error("device index out of range"); return SIFT3D_ERR_ARG; }
	S3D_HIP(hipSetDevice(device));
	return SIFT3D_OK;
}

static void free_lists(sift3d_ctx *c) {
	hipFree(c->d_ext); c->d_ext = nullptr;
	hipFree(c->d_codes); c->d_codes = nullptr;
	hipFree(c->d_order); c->d_order = nullptr;
	hipFree(c->d_kpout); c->d_kpout = nullptr;
	hipFree(c->d_desc); c->d_desc = nullptr;
	hipFree(c->d_xyz); c->d_xyz = nullptr;
	hipFree(c->d_prov); c->d_prov = nullptr;
	hipFree(c->d_prov2); c->d_prov2 = nullptr;
	hipFree(c->dsplit.gacc); c->dsplit = DescSplit{};
	hipFree(c->d_refined); c->d_refined = nullptr; c->refined_cap = 0;
}

int alloc_lists(sift3d_ctx *c, unsigned ext_cap) {
	free_lists(c);
	c->ext_cap = ext_cap;
	c->kp_cap = ext_cap;  // every extremum could survive orientation
	S3D_HIP(hipMalloc(&c->d_ext, sizeof(DevKp) * (size_t)c->ext_cap));
	S3D_HIP(hipMalloc(&c->d_codes, sizeof(int) * (size_t)c->ext_cap));
	S3D_HIP(hipMalloc(&c->d_order, sizeof(int) * (size_t)c->kp_cap));
	S3D_HIP(hipMalloc(&c->d_kpout, sizeof(sift3d_keypoint) * (size_t)c->kp_cap));
	S3D_HIP(hipMalloc(&c->d_desc, sizeof(float) * kDesc * (size_t)c->kp_cap));
	S3D_HIP(hipMalloc(&c->d_xyz, sizeof(float) * 3 * (size_t)c->kp_cap));
	{
		// split descriptor windows: [cap][768] int accumulators | [cap][8] masses | [cap] arrivals (zeroed once: every run leaves them clean)
		const unsigned scap = 4096;
		const size_t words = (size_t)scap * (kDesc + 8 + 1);
		int *base = nullptr;
		S3D_HIP(hipMalloc(&base, sizeof(int) * words));
		// on the handle's own stream: the legacy null stream would synchronise with every blocking stream of the host application
		hipError_t me = hipMemsetAsync(base, 0, sizeof(int) * words, c->stream);
		if (me == hipSuccess) me = hipStreamSynchronize(c->stream);
		if (me != hipSuccess) {
			hipFree(base);
			set_last_error(std::string("HIP error: ") + hipGetErrorString(me) + " (clearing the split-window scratch)");
			return SIFT3D_ERR_HIP;
		}
		c->dsplit.gacc = base;
		c->dsplit.gmass = reinterpret_cast<float *>(base + (size_t)scap * kDesc);
		c->dsplit.gdone = reinterpret_cast<unsigned *>(base + (size_t)scap * (kDesc + 8));
		c->dsplit.cap = scap;
	}
	S3D_HIP(hipMalloc(&c->d_prov, sizeof(unsigned) * ((size_t)c->ext_cap + 1)));
	c->det.prov = c->d_prov; c->det.prov_count = c->d_prov + c->ext_cap; c->det.prov_cap = c->ext_cap;
	if (c->det_o.size() > 1) {  // octaves >= 1: equal slices of a second parking list, each followed by its counter
		const size_t n2 = c->det_o.size() - 1;
		const unsigned slice = std::max(64u, (unsigned)(c->ext_cap / n2));
		S3D_HIP(hipMalloc(&c->d_prov2, sizeof(unsigned) * ((size_t)slice + 1) * n2));
		for (size_t o = 1; o < c->det_o.size(); o++) {
			c->det_o[o].prov = c->d_prov2 + (o - 1) * ((size_t)slice + 1);
			c->det_o[o].prov_count = c->det_o[o].prov + slice;
			c->det_o[o].prov_cap = slice;
		}
	}
	return SIFT3D_OK;
}

extern "C" void sift3d_default_params(sift3d_params *p) {
	if (!p) return;
	p->num_kp_levels = 3;
	p->sigma_default = 1.6f;
	p->sigma_n_default = 1.15f;
	p->peak_thresh = 0.1f;
	p->max_eig_thres = 0.9f;
	p->corner_thresh = 0.4f;
}

// No reference counterpart (generalises IsExtrema_neighbor, Src/cSIFT3D.cc:884-911): the reference's 8-neighbour rule, no fit
extern "C" void sift3d_default_detect_options(sift3d_detect_options *o) {
	if (!o) return;
	memset(o, 0, sizeof(*o));
	o->neighbours = 8;
	o->refine = 0;
	o->max_offset = 0.5f;
	o->contrast_thresh = 0.0f;
	o->edge_ratio = 0.0f;
}

extern "C" int sift3d_device_count(int *n) {
	int k = 0;
	if (hipGetDeviceCount(&k) != hipSuccess) k = 0;
	if (n) *n = k;
	return SIFT3D_OK;
}

extern "C" const char *sift3d_error_string(int code) {
	switch (code) {
	case SIFT3D_OK: return "ok";
	case SIFT3D_ERR_ARG: return "bad argument";
	case SIFT3D_ERR_NO_DEVICE: return "no usable HIP device (no CPU fallback)";
	case SIFT3D_ERR_HIP: return "HIP runtime error";
	case SIFT3D_ERR_STATE: return "call out of order";
	case SIFT3D_ERR_CAPACITY: return "device list capacity exceeded";
	default: return "unknown error";
	}
}

extern "C" const char *sift3d_last_error(void) { return g_last_error.c_str(); }

extern "C" int sift3d_destroy(sift3d_handle c) {
	if (!c) return SIFT3D_OK;
	hipSetDevice(c->device);
	c->pending = false;  // (an asynchronous run in flight is drained below, its results dropped)
	if (c->uploader.joinable()) c->uploader.join();  // (a constructor that failed beside its upload)
	if (c->up_stream) { hipStreamSynchronize(c->up_stream); hipStreamDestroy(c->up_stream); c->up_stream = nullptr; }
	if (c->stream) hipStreamSynchronize(c->stream);
	if (c->own_stream && c->own_stream != c->stream) hipStreamSynchronize(c->own_stream);
	free_lists(c);
	if (!c->ext_arena) hipFree(c->arena);
	hipFree(c->in_own);
	hipFree(c->in_raw);
	hipFree(c->d_peer);
	hipFree(c->d_words);
	if (c->h_words) (void)hipHostFree(c->h_words);
	hipFree(c->d_slots_part);
	hipFree(c->det.masks); hipFree(c->det.block_counts); hipFree(c->det.block_offsets);
	hipFree(c->d_masks2); hipFree(c->d_counts2); hipFree(c->d_offsets2);
	if (c->ev_det_fork) hipEventDestroy(c->ev_det_fork);
	if (c->ev_det_join) hipEventDestroy(c->ev_det_join);
	if (c->ev_det_join2) hipEventDestroy(c->ev_det_join2);
	hipFree(c->d_levels); hipFree(c->d_luts); hipFree(c->d_lutpool);
	for (auto &e : c->ev) if (e) hipEventDestroy(e);
	for (auto &e : c->ev_seed) if (e) hipEventDestroy(e);
	for (auto &e : c->ev_done) if (e) hipEventDestroy(e);
	if (c->ev_fork) hipEventDestroy(c->ev_fork);
	for (size_t o = 1; o < c->ostream.size(); o++) if (c->ostream[o] && c->ostream[o] != c->stream && c->ostream[o] != c->own_stream) hipStreamDestroy(c->ostream[o]);
	if (c->cstream) hipStreamDestroy(c->cstream);
	if (c->own_stream) hipStreamDestroy(c->own_stream);
	delete c;
	return SIFT3D_OK;
}

// Initialize + Initialize_Pyramid geometry, Src/cSIFT3D.cc:237-266, Src/cUtil.cc:177-235
static int octaves_of(int nx, int ny, int nz) {  // Src/cSIFT3D.cc:254-255
	const int mn = std::min(nx, std::min(ny, nz));
	return std::max(0, (int)log2f((float)mn) - 3 + 1);
}

float level_scale(const sift3d_params &p, int octave, int s) {
	const double sigma0 = (double)p.sigma_default * pow(2.0, -1.0 / 3.0);
	const double scale_factor = pow(2.0, (double)octave + (double)s / (double)p.num_kp_levels);
	return (float)(scale_factor * sigma0);
}

void plan_pyramid(sift3d_ctx *c, int noct_total) {
	c->noct = noct_total >= 0 ? std::max(0, noct_total - c->octave_base) : octaves_of(c->nx, c->ny, c->nz);
	if (c->slab) c->noct = std::min(c->noct, 1);
	c->ng = c->p.num_kp_levels + 3;
	c->nd = c->p.num_kp_levels + 2;
	c->gss.assign((size_t)c->noct * c->ng, Level());
	c->dog.assign((size_t)c->noct * c->nd, Level());
	for (int pyr = 0; pyr < 2; pyr++) {
		const int interval = pyr ? c->nd : c->ng;
		std::vector<Level> &P = pyr ? c->dog : c->gss;
		int nx = c->nx, ny = c->ny, nz = c->nz;
		float u = (float)(1 << c->octave_base);  // units double per octave starting at 1 (Src/cUtil.cc:215-225)
		for (int o = 0; o < c->noct; o++) {
			for (int s = 0; s < interval; s++) {
				Level &L = P[(size_t)o * interval + s];
				L.nx = nx; L.ny = ny; L.nz = nz; L.unit = u;
				L.scale = level_scale(c->p, o + c->octave_base, s);
				if (c->slab) { L.bz = c->own1 - c->own0 + 2 * c->halo; L.zoff = c->own0 - c->halo; }
			}
			nx /= 2; ny /= 2; nz /= 2;
			u *= 2;
		}
	}
}

int upload_luts(sift3d_ctx *c, const std::vector<WinLut> &luts, std::vector<float> &pool) {
	if (pool.empty()) pool.push_back(-1.0f);
	if (c->d_luts) { S3D_HIP(hipFree(c->d_luts)); c->d_luts = nullptr; }
	if (c->d_lutpool) { S3D_HIP(hipFree(c->d_lutpool)); c->d_lutpool = nullptr; }
	S3D_HIP(hipMalloc(&c->d_luts, sizeof(WinLut) * luts.size()));
	S3D_HIP(hipMalloc(&c->d_lutpool, sizeof(float) * pool.size()));
	S3D_HIP(hipMemcpy(c->d_luts, luts.data(), sizeof(WinLut) * luts.size(), hipMemcpyHostToDevice));
	S3D_HIP(hipMemcpy(c->d_lutpool, pool.data(), sizeof(float) * pool.size(), hipMemcpyHostToDevice));
	return SIFT3D_OK;
}

std::vector<WinLut> blank_luts(const sift3d_ctx *c) {
	std::vector<WinLut> luts((size_t)std::max(1, c->noct + c->octave_base) * 8 * 2);
	for (auto &l : luts) { l.off = 0; l.len = 0; l.nin = -1; l.radius = 0; l.sigma = 0; l.fix_scale = 1.0f; l.wsum = 1.0f; l.list_off = -1; l.list_R = 0; }
	return luts;
}

static int build_luts(sift3d_ctx *c) {
	std::vector<WinLut> luts = blank_luts(c);
	std::vector<float> pool;
	for (int o = 0; o < c->noct; o++)
		for (int lv = 1; lv <= c->p.num_kp_levels && lv < 8; lv++) {
			const Level &D = c->dog[(size_t)o * c->nd + lv];  // keypoint scale = DoG level scale (Src/cSIFT3D.cc:407)
			const float u = D.unit, scale = D.scale;
			for (int which = 0; which < 2; which++) {
				float sigma, radius;
				if (which == 0) { sigma = 1.5f * scale; radius = sigma * 3.0f; }
				else { sigma = scale * 7.071067812f; radius = 2.0f * sigma; }
				if (!append_lut(pool, luts[((size_t)(o + c->octave_base) * 8 + lv) * 2 + which], which, sigma, radius, u, scale)) c->desc_lut_lds = false;
			}
		}
	return upload_luts(c, luts, pool);
}

static size_t al64(size_t n) { return (n + 63) & ~(size_t)63; }

// floats needed for: input | per-octave scratch A,B | GSS levels | DoG levels
size_t arena_floats_of(const sift3d_ctx *c) {
	size_t total = c->in_own ? 0 : al64(c->in.n());
	if (!c->slab) for (int o = 0; o < c->noct; o++) total += 2 * al64(c->gss[(size_t)o * c->ng].n());  // slabs only run the fused kernel
	for (auto &L : c->gss) total += al64(L.n());
	for (auto &L : c->dog) total += al64(L.n());
	return total;
}

// The heads of the octaves >= 1 gain from one in-order chain stream only where they are short launches: volumes of at most 4 M voxels
static bool chain_stream_fits(const sift3d_ctx *c) { return (size_t)c->nx * c->ny * c->nz <= ((size_t)1 << 22); }

int create_common(sift3d_handle *out, const CreateCfg &cfg, const sift3d_params *params, int device) {
	*out = nullptr;
	if (cfg.nx <= 0 || cfg.ny <= 0 || cfg.nz <= 0) { set_last_error("bad dimensions"); return SIFT3D_ERR_ARG; }
	int rc = set_device(device);
	if (rc) return rc;
	sift3d_ctx *c = new sift3d_ctx();
	c->device = device;
	if (params) c->p = *params; else sift3d_default_params(&c->p);
	sift3d_default_detect_options(&c->dopt);
	if (c->p.num_kp_levels < 1 || c->p.num_kp_levels > 5) { delete c; set_last_error("num_kp_levels must be in [1,5]"); return SIFT3D_ERR_ARG; }
	c->nx = cfg.nx; c->ny = cfg.ny; c->nz = cfg.nz;
	c->octave_base = cfg.octave_base; c->seeded = cfg.seeded;
	c->slab = cfg.slab; c->own0 = cfg.z0; c->own1 = cfg.z1; c->halo = cfg.halo;
	c->use_fused = !hook(SIFT3D_HOOK_SEPARABLE);
	plan_pyramid(c, cfg.noct_total);
	c->in.nx = cfg.nx; c->in.ny = cfg.ny; c->in.nz = cfg.nz; c->in.unit = (float)(1 << c->octave_base); c->in.scale = 1.f;
	if (c->slab) { c->in.bz = c->own1 - c->own0 + 2 * c->halo; c->in.zoff = c->own0 - c->halo; }
	if (c->seeded) c->in.bz = 1;  // no input volume: keep a token plane
	for (auto &L : c->gss) if ((size_t)L.nx * L.ny * L.planes() >= ((size_t)1 << 31)) { delete c; set_last_error("level too large for int32 voxel indices"); return SIFT3D_ERR_ARG; }

	// host tables
	std::vector<float> sig;
	float base_sigma;
	level_sigmas(c->p, sig, base_sigma);
	c->taps.resize(c->ng);
	bool ok = build_taps(base_sigma, c->base_taps);
	for (int i = 1; i < c->ng; i++) ok = ok && build_taps(sig[i], c->taps[i]);
	if (!ok) { delete c; set_last_error("Gaussian kernel wider than the supported 129 taps"); return SIFT3D_ERR_ARG; }

#define CHECKED(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { set_last_error(std::string(#call) + ": " + hipGetErrorString(e_)); sift3d_destroy(c); return SIFT3D_ERR_HIP; } } while (0)
	CHECKED(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
	for (auto &e : c->ev) CHECKED(hipEventCreate(&e));
	CHECKED(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
	c->ostream.assign((size_t)std::max(1, c->noct), nullptr);
	c->ev_seed.assign(c->ostream.size(), nullptr);
	c->ev_done.assign(c->ostream.size(), nullptr);
	c->own_stream = c->stream;
	c->ostream[0] = c->stream;
	if (cfg.host_volume && !cfg.ext_arena && !c->slab && !c->seeded) {
		const size_t V0 = c->in.n();
		CHECKED(hipMalloc(&c->in_own, sizeof(float) * al64(V0)));
		CHECKED(hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking));
		const void *vol = cfg.host_volume;
		// integer voxels (sift3d_create_typed) travel at their own width into a buffer of their own
		const size_t bytes = (size_t)dtype_bytes(cfg.host_dtype) * V0;
		if (cfg.host_dtype != SIFT3D_DT_F32) CHECKED(hipMalloc(&c->in_raw, bytes));
		void *dst = c->in_raw ? c->in_raw : static_cast<void *>(c->in_own);
		// (measured, 512^3: 14.5 ms with the copy behind the allocations, 15.6 with its own buffer but no thread, 12.0 like this)
		c->uploader = std::thread([c, vol, dst, bytes, device] {
			int r = set_device(device);
			if (r == SIFT3D_OK) r = staged_h2d(dst, vol, bytes, device, c->up_stream);
			if (r != SIFT3D_OK) c->upload_err = sift3d_last_error();  // (the error text is thread-local)
			c->upload_rc = r;
		});
	}
	// SIFT3D_HOOK_ONE_STREAM (profiling): every octave on the main stream, so a kernel trace shows isolated launch durations
	const bool one_stream = hook(SIFT3D_HOOK_ONE_STREAM) != 0;
	for (size_t o = 0; o < c->ostream.size(); o++) {
		if (o > 0 && one_stream) c->ostream[o] = c->stream;
		else if (o > 0) CHECKED(hipStreamCreateWithFlags(&c->ostream[o], hipStreamNonBlocking));
		// the chain stream, only for the volumes whose plan uses it (plan_run): HIP deals streams onto its hardware queues in creation
		// order, so one more stream changes which octave streams share a queue (docs/experiments.md, "One stream more")
		if (o == 1 && !one_stream && !c->slab && chain_stream_fits(c)) CHECKED(hipStreamCreateWithFlags(&c->cstream, hipStreamNonBlocking));
		CHECKED(hipEventCreateWithFlags(&c->ev_seed[o], hipEventDisableTiming));
		CHECKED(hipEventCreateWithFlags(&c->ev_done[o], hipEventDisableTiming));
	}

	// ---- arena: input | per-octave scratch A,B | GSS levels | DoG levels (each 256-B aligned) ----
	const size_t total = arena_floats_of(c);
	c->arena_floats = total;
	if (cfg.ext_arena) {
		if (cfg.ext_arena_floats < total) { set_last_error("caller arena too small"); sift3d_destroy(c); return SIFT3D_ERR_ARG; }
		c->arena = cfg.ext_arena;
		c->ext_arena = true;
	} else {
		CHECKED(hipMalloc(&c->arena, sizeof(float) * total));
	}
	float *p = c->arena;
	if (c->in_own) c->in.d = c->in_own;
	else { c->in.d = p; p += al64(c->in.n()); }
	c->tmpA.assign((size_t)std::max(1, c->noct), nullptr);
	c->tmpB.assign((size_t)std::max(1, c->noct), nullptr);
	for (int o = 0; o < c->noct && !c->slab; o++) {
		const size_t vo = al64(c->gss[(size_t)o * c->ng].n());
		c->tmpA[o] = p; p += vo;
		c->tmpB[o] = p; p += vo;
	}
	for (auto &L : c->gss) { L.d = p; p += al64(L.n()); }
	for (auto &L : c->dog) { L.d = p; p += al64(L.n()); }

	const size_t nwords = 1 + (size_t)std::max(1, c->noct * c->nd) + 8 + 1;  // ... + total, overflow, nkp, describe work counter, describe redo counter, orientation redo counter; the last word: non-finite input flag
	CHECKED(hipMalloc(&c->d_words, sizeof(unsigned) * nwords));
	CHECKED(hipMemset(c->d_words, 0, sizeof(unsigned) * nwords));
	CHECKED(hipHostMalloc(&c->h_words, sizeof(unsigned) * 8, hipHostMallocDefault));
	CHECKED(hipMalloc(&c->d_slots_part, sizeof(unsigned) * slots_scratch_words()));
	c->d_inmax = c->d_words;
	c->d_dogmax = c->d_words + 1;
	c->d_total = c->d_words + 1 + std::max(1, c->noct * c->nd);  // [0] extrema total, [1] overflow flag
	c->d_nkp = c->d_total + 2;

	// detection scratch sized for the first octave (the largest): one ballot word per 64 voxels of a row, one count per 16 rows
	const int scan_planes = c->slab ? (c->own1 - c->own0) : cfg.nz;
	{
		const size_t kl = (size_t)c->p.num_kp_levels;
		const size_t words = kl * (size_t)scan_planes * cfg.ny * ((cfg.nx + 63) / 64);
		c->det_blocks = kl * (size_t)scan_planes * ((cfg.ny + 15) / 16);
		CHECKED(hipMalloc(&c->det.masks, sizeof(unsigned long long) * std::max<size_t>(words, 1)));
		CHECKED(hipMalloc(&c->det.block_counts, sizeof(unsigned) * std::max<size_t>(c->det_blocks, 1)));
		CHECKED(hipMalloc(&c->det.block_offsets, sizeof(unsigned) * std::max<size_t>(c->det_blocks, 1)));
	}
	c->det.total = c->d_total;
	{
		const bool det_serial = hook(SIFT3D_HOOK_DET_SERIAL) != 0;
		if (!c->slab && c->noct > 1 && !det_serial && c->ostream.size() > 1 && c->ostream[1] != c->stream) {
			const size_t kl = (size_t)c->p.num_kp_levels;
			c->det_o.assign((size_t)c->noct, DetectBufs{});
			size_t words = 0, blocks = 0;
			std::vector<size_t> woff((size_t)c->noct, 0), boff((size_t)c->noct, 0);
			for (int o = 1; o < c->noct; o++) {
				const Level &D = c->dog[(size_t)o * c->nd + 1];
				woff[(size_t)o] = words; boff[(size_t)o] = blocks;
				words += kl * (size_t)D.nz * D.ny * ((D.nx + 63) / 64);
				blocks += kl * (size_t)D.nz * ((D.ny + 15) / 16);
			}
			CHECKED(hipMalloc(&c->d_masks2, sizeof(unsigned long long) * std::max<size_t>(words, 1)));
			CHECKED(hipMalloc(&c->d_counts2, sizeof(unsigned) * std::max<size_t>(blocks, 1)));
			CHECKED(hipMalloc(&c->d_offsets2, sizeof(unsigned) * std::max<size_t>(blocks, 1)));
			for (int o = 1; o < c->noct; o++) {
				DetectBufs &b = c->det_o[(size_t)o];
				b.masks = c->d_masks2 + woff[(size_t)o]; b.block_counts = c->d_counts2 + boff[(size_t)o];
				b.block_offsets = c->d_offsets2 + boff[(size_t)o]; b.total = c->d_total;
			}
			CHECKED(hipEventCreateWithFlags(&c->ev_det_fork, hipEventDisableTiming));
			CHECKED(hipEventCreateWithFlags(&c->ev_det_join, hipEventDisableTiming));
			CHECKED(hipEventCreateWithFlags(&c->ev_det_join2, hipEventDisableTiming));
		}
	}

	// level table for the keypoint kernels, indexed by ABSOLUTE octave
	std::vector<LevelRef> lr((size_t)std::max(1, c->noct + c->octave_base) * 8, LevelRef{nullptr, 0, 0, 0, 1.f, 0});
	for (int o = 0; o < c->noct; o++)
		for (int i = 0; i < c->ng && i < 8; i++) {
			const Level &L = c->gss[(size_t)o * c->ng + i];
			lr[(size_t)(o + c->octave_base) * 8 + i] = LevelRef{L.d, L.nx, L.ny, L.nz, L.unit, L.zoff};
		}
	CHECKED(hipMalloc(&c->d_levels, sizeof(LevelRef) * lr.size()));
	CHECKED(hipMemcpy(c->d_levels, lr.data(), sizeof(LevelRef) * lr.size(), hipMemcpyHostToDevice));
	rc = build_luts(c);
	if (rc) { sift3d_destroy(c); return rc; }
	FaceConst faces[kFaces];
	build_faces(faces);
	FaceSym sym;
	if (!build_facesym(faces, &sym)) { set_last_error("icosahedron symmetry table: no matching face"); sift3d_destroy(c); return SIFT3D_ERR_STATE; }
	CHECKED(upload_faces(faces, &sym));

	// keypoint lists: synthetic blob volumes give ~6e-4*V extrema; leave 8x headroom, regrow on overflow
	const size_t V0 = (size_t)cfg.nx * cfg.ny * scan_planes;
	unsigned cap = (unsigned)std::min<size_t>(std::max<size_t>(4096, V0 / 256), 4u << 20);
	if (hook(SIFT3D_HOOK_LIST_CAP) > 0) cap = (unsigned)hook(SIFT3D_HOOK_LIST_CAP);  // tests: overflow -> regrow -> rerun
	rc = alloc_lists(c, cap);
	if (rc) { sift3d_destroy(c); return rc; }
	CHECKED(hipStreamSynchronize(c->stream));
#undef CHECKED
	{
		// first create on this device: load the kernels of every translation unit now (HIP loads a unit's code object at the first
		// launch of one of its kernels: ~1 ms of the first KpSiftAlgorithm of a process went there, scripts/step_times_probe.py)
		static std::atomic<unsigned long long> loaded{0};
		const unsigned long long bit = 1ull << (device & 63);
		if (!(loaded.fetch_or(bit) & bit)) { preload_march_kernels(); preload_small_kernels(); preload_detect_kernels(); preload_orient_kernels(); preload_desc_kernels(); preload_match_kernels(); preload_ingest_kernels(); }
	}
	*out = c;
	return SIFT3D_OK;
}

int join_upload(sift3d_ctx *c) {
	if (c->uploader.joinable()) c->uploader.join();
	if (c->upload_rc != SIFT3D_OK) { set_last_error(c->upload_err); return c->upload_rc; }
	S3D_HIP(hipStreamSynchronize(c->up_stream));  // every chunk has landed: the kernels behind it run on the handle's stream
	return SIFT3D_OK;
}

extern "C" int sift3d_create(sift3d_handle *out, const float *volume, int nx, int ny, int nz, const sift3d_params *params,
                             int device, int volume_on_device) {
	if (!out || !volume || nx <= 0 || ny <= 0 || nz <= 0) { set_last_error("sift3d_create: bad argument"); return SIFT3D_ERR_ARG; }
	if ((size_t)nx * ny * nz >= ((size_t)1 << 31)) { set_last_error("volume too large for int32 voxel indices"); return SIFT3D_ERR_ARG; }
	CreateCfg cfg;
	cfg.nx = nx; cfg.ny = ny; cfg.nz = nz;
	if (!volume_on_device) cfg.host_volume = volume;  // its upload starts inside create_common, beside the allocations
	int rc = create_common(out, cfg, params, device);
	if (rc) return rc;
	sift3d_ctx *c = *out;
	// ---- constructor work proper: copy + data_scale (Src/cSIFT3D.cc:161-162) ----
	const size_t V0 = (size_t)nx * ny * nz;
	hipError_t e = hipSuccess;
	if (volume_on_device) e = hipMemcpyAsync(c->in.d, volume, sizeof(float) * V0, hipMemcpyDeviceToDevice, c->stream);
	else if ((rc = join_upload(c)) != SIFT3D_OK) { sift3d_destroy(c); *out = nullptr; return rc; }
	if (e == hipSuccess) {
		unsigned *d_nonfinite = c->d_words + 1 + (size_t)std::max(1, c->noct * c->nd) + 8;
		launch_absmax(c->in.d, V0, c->d_inmax, c->stream, d_nonfinite);
		launch_scale_by_max(c->in.d, V0, c->d_inmax, c->stream);
		// A volume with a NaN or Inf voxel (k_absmax's flag; four bytes read behind the synchronisation this constructor ends with anyway)
		// takes the generic three-pass kernels in their `exact` form for every Gaussian level, the last one included (no k_lazy_next): the
		// fused, the one-workgroup and the lazy kernels use the interior shortcut tap * src[p - d], which is the reference's arithmetic on
		// finite data only.  (The first and the last DoG level stay elided as in any run: the extremum test forms them as (hi - lo) * (-1)
		// from the two Gaussian levels, the arithmetic of the stored levels.)
		e = hipMemcpyAsync(&c->h_words[7], d_nonfinite, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
		if (e == hipSuccess && c->h_words[7] != 0) { c->nonfinite = true; c->use_fused = false; }
	}
	if (e == hipSuccess) e = hipGetLastError();
	if (e != hipSuccess) { set_last_error(hipGetErrorString(e)); sift3d_destroy(c); *out = nullptr; return SIFT3D_ERR_HIP; }
	return SIFT3D_OK;
}

// GaussianSmooth_3D (Src/cSIFT3D.cc:535-622) on device buffers: X -> Y -> Z(+DoG)
#ifndef S3D_FUSED_MIN_DEFAULT
#define S3D_FUSED_MIN_DEFAULT 33  /* levels with a dimension <= 32 (octaves 4+ of a 512^3 volume) take the generic separable kernels */
#endif
#ifndef S3D_O0_TAIL_SLOTS_DEFAULT
#define S3D_O0_TAIL_SLOTS_DEFAULT 512
#endif
#ifndef S3D_BG_SLOTS_DEFAULT
#define S3D_BG_SLOTS_DEFAULT 256
#endif
// One level of octave o on stream st, with the wave priority and the slot plan the RunPlan gives its part of the octave.
// half_out (optional): level 0 of the next octave; returns true when the march kernel wrote it together with dst (the caller then
// skips the decimation launch)
static bool smooth_level(sift3d_ctx *c, int o, hipStream_t st, int prio, int plan_slots, const float *src, const Level &dst, const Taps &t,
                         const float *prev, float *dog, unsigned *dogmax, const Level *half_out = nullptr) {
	// hot path: one fused pass (x, y, z blur + DoG + abs-max; kernels_march.hip); prev == src for every DoG-producing level.
	// The plane size decides, not the depth: a thin volume marches its few planes like any other chunk; launch_march_level declines a
	// level whose column is shorter than its kernel (nz < 2 hw + 2), which then takes the separable passes.
	static const int fused_min = dev_tune_i("S3D_FUSED_MIN", S3D_FUSED_MIN_DEFAULT);
	if (c->use_fused && (prev == nullptr || prev == src) && std::min(dst.nx, dst.ny) >= fused_min) {
		MarchHalf hf;
		// (the seed level's kernel also writes level 0 of the next octave: no decimation launch on the octave -> octave chain)
		const bool want_half = half_out != nullptr && march_half_ok(dst.nx, dst.ny, dst.zr_all());
		if (want_half) { hf.d = half_out->d; hf.nx = half_out->nx; hf.ny = half_out->ny; hf.nz = half_out->nz; }
		if (launch_march_level(src, dst.d, dog, dogmax, dst.nx, dst.ny, dst.zr_all(), t, st, plan_slots, prio, want_half ? &hf : nullptr))
			return want_half;
	}
	launch_conv_axis(0, src, c->tmpA[o], dst.nx, dst.ny, dst.nz, t, nullptr, nullptr, nullptr, st, c->nonfinite);
	launch_conv_axis(1, c->tmpA[o], c->tmpB[o], dst.nx, dst.ny, dst.nz, t, nullptr, nullptr, nullptr, st, c->nonfinite);
	launch_conv_axis(2, c->tmpB[o], dst.d, dst.nx, dst.ny, dst.nz, t, prev, dog, dogmax, st, c->nonfinite);
	return false;
}

// the detection table of the context's octave slot o (a slab context holds one octave: o = 0): DoG levels 1 .. nd-2 (Src/cSIFT3D.cc:376)
// and, where the run elides them, the Gaussian levels that stand in for DoG[0], DoG[nd-1] and the lazy last Gaussian level
void fill_detect_levels(const sift3d_ctx *c, int o, DetectLevels &DL) {
	memset(&DL, 0, sizeof(DL));
	const Level *G = &c->gss[(size_t)o * c->ng], *D = &c->dog[(size_t)o * c->nd];
	const int nl = c->nd - 2;
	for (int i = 1; i <= nl; i++) {
		DL.cur[i - 1] = D[i].d; DL.prev[i - 1] = D[i - 1].d; DL.next[i - 1] = D[i + 1].d;
		DL.absmax_bits[i - 1] = c->d_dogmax + (size_t)o * c->nd + i;
		DL.level_id[i - 1] = i;
		DL.scale[i - 1] = D[i].scale;
	}
	if (c->dog_elide) {
		DL.prev0_hi = G[1].d; DL.prev0_lo = G[0].d;
		DL.nextl_hi = G[c->nd].d; DL.nextl_lo = G[c->nd - 1].d;
		DL.nextl_slot = nl - 1;
		if (c->g_last_elide) { DL.nextl_hi = nullptr; DL.lazy_src = DL.nextl_lo; }
	}
}

// the DoG levels launch_refine reads, every octave of the context
static void fill_dog_table(const sift3d_ctx *c, DogTable &T) {
	memset(&T, 0, sizeof(T));
	T.octave_base = c->octave_base;
	for (int o = 0; o < c->noct && o < kDogTabOct; o++) {
		const Level &D0 = c->dog[(size_t)o * c->nd];
		T.nx[o] = D0.nx; T.ny[o] = D0.ny;
		for (int i = 0; i < c->nd && i < kDogTabLv; i++) T.d[o][i] = c->dog[(size_t)o * c->nd + i].d;
	}
}

// ---- the schedule of a run (RunPlan, ctx_internal.h; DESIGN.md, "The schedule of a run"; measurements: docs/experiments.md) ----
// The SMALL octaves (16^3-class and below) run in ONE launch of one workgroup that keeps the octave in LDS (kernels_small.hip) instead
// of ~16 launches of a few microseconds per octave on the stage's critical chain: the first octave of that launch, -1 for none, and
// the launch's arguments
static void plan_small_launch(const sift3d_ctx *c, RunPlan &plan) {
	plan.small_first = -1;
	unsigned build_mask = 0, dog_mask = 0;
	int max_hw = 0;
	bool ok = c->use_fused && !c->slab && c->ng <= kSmallMaxLv;
	for (int i = 1; i < c->ng && ok; i++) {
		if (c->g_last_elide && i == c->ng - 1) continue;
		build_mask |= 1u << i;
		if (!(c->dog_elide && (i - 1 == 0 || i - 1 == c->nd - 1))) dog_mask |= 1u << (i - 1);
		const Taps &t = c->taps[i];
		for (int d = 1; d <= t.hw && ok; d++) ok = memcmp(&t.w[t.hw + d], &t.w[t.hw - d], sizeof(float)) == 0;  // symmetric bit for bit
		max_hw = std::max(max_hw, t.hw);
	}
	if (!ok || small_padded_hw(max_hw) <= 0) return;
	auto fits = [&](int o) { const Level &L = c->gss[(size_t)o * c->ng]; return small_octave_fits(L.nx, L.ny, L.nz, max_hw); };
	int first = -1;
	for (int o = 0; o < c->noct && first < 0; o++) if (c->noct - o <= kSmallMaxOct && fits(o)) first = o;
	// EVERY octave of the launch must satisfy hw <= n - 2 (the extended-line form of the boundary rule): the octaves behind the first
	// are smaller, which makes the capacity limits easier and THIS one harder (sigma_default 1.7: hw 7 at the 8^3 octave of a
	// power-of-two volume; the glast_eager hook: hw 8).  One that fails sends the whole chain down the separable kernels.
	for (int o = first; first >= 0 && o < c->noct; o++) if (!fits(o)) first = -1;
	if (first < 0) return;
	plan.small_first = first;
	SmallArgs &sa = plan.small;
	memset(&sa, 0, sizeof(sa));
	sa.noct = c->noct - first; sa.ng = c->ng; sa.nd = c->nd; sa.seed = c->p.num_kp_levels;
	sa.build_mask = build_mask; sa.dog_mask = dog_mask;
	sa.dogmax = c->d_dogmax + (size_t)first * c->nd;
	sa.hwp = small_padded_hw(max_hw);
	for (int i = 1; i < c->ng; i++) {
		const Taps &t = c->taps[i];
		if (t.hw > sa.hwp) continue;  // (a level the launch does not build)
		for (int k = 0; k <= sa.hwp; k++) sa.w[i][k] = k >= sa.hwp - t.hw ? t.w[k - (sa.hwp - t.hw)] : 0.0f;
	}
	for (int o = first; o < c->noct; o++) {
		SmallOct &so = sa.oct[o - first];
		const Level &L = c->gss[(size_t)o * c->ng];
		so.nx = L.nx; so.ny = L.ny; so.nz = L.nz;
		for (int i = 0; i < c->ng; i++) so.g[i] = c->gss[(size_t)o * c->ng + i].d;
		for (int i = 0; i < c->nd; i++) so.dog[i] = c->dog[(size_t)o * c->nd + i].d;
	}
}

// Streams, wave priority and slot plan of every octave's head and tail
static void plan_octaves(const sift3d_ctx *c, RunPlan &plan) {
	static const int tail_slots = dev_tune_i("S3D_O0_TAIL_SLOTS", S3D_O0_TAIL_SLOTS_DEFAULT);
	static const int bg_slots = dev_tune_i("S3D_BG_SLOTS", S3D_BG_SLOTS_DEFAULT);
	const int sf = plan.small_first;
	plan.chain = c->cstream != nullptr;  // (create_common: volumes of at most 4 M voxels, chain_stream_fits)
	plan.oct.assign((size_t)std::max(1, c->noct), RunPlan::Oct{});
	for (int o = 0; o < c->noct; o++) {
		RunPlan::Oct &oc = plan.oct[(size_t)o];
		const bool in_small = sf >= 0 && o >= sf;
		// the octaves of the small launch share the stream of the first of them; with a chain stream the heads of the octaves >= 1
		// and the small launch run on it, in order: a dependency across streams costs 13-16 us, consecutive launches of one stream none
		const int own = in_small ? sf : o;
		oc.head = plan.chain && o >= 1 ? kChainStream : own;
		oc.tail = plan.chain && o >= 1 && in_small ? kChainStream : own;
		// HIP deals the streams onto its hardware queues in the pattern 1 2 3 4 4 3 2 1: with the small launch on the fourth stream the
		// tail of the octave above it would queue BEHIND that launch; it goes to the stream of the octave above, idle by then
		oc.tail_moved = sf >= 3 && o == sf - 1 && !plan.chain;
		if (oc.tail_moved) oc.tail = o - 1;
		// Single-round launches keep every slot they take until they end: the tail of octave 0 leaves a third of the machine to the
		// chains of the smaller octaves, which are planned for that third and run at the top wave priority (each waits for the seed
		// level of the one above, and beside the big launches their workgroups crawl)
		oc.prio = c->noct > 1 && o >= 1 ? 2 : 0;
		oc.head_slots = c->noct > 1 && o >= 1 ? bg_slots : 0;
		oc.tail_slots = c->noct > 1 ? (o == 0 ? tail_slots : bg_slots) : 0;
	}
}

// Detection: the masks of octave 0, octave 1 and the octaves >= 2 on up to three streams, one ordered compaction
static void plan_detect(const sift3d_ctx *c, int upto, RunPlan &plan) {
	plan.det_two = upto >= 3 && c->det_o.size() > 1;
	// det_o exists only where create_common gave octave 1 a stream of its own (noct > 1, no one_stream / det_serial hook, no slab), and
	// sift3d_set_stream only replaces entries equal to the handle's stream: with a second scratch every ostream[o] is distinct
	plan.det_early = plan.det_two;
	plan.det_rest_stream = !plan.det_two ? 0 : (c->noct > 2 ? 2 : 1);
	// the masks of an octave >= 2 follow ITS pyramid (the event its last level recorded), not every octave's
	plan.det_rest_own = plan.det_early && plan.det_rest_stream == 2;
	// one scan + one emit launch for all octaves; k_emit_multi's table holds eight: a ninth octave keeps octave 0's own launches in
	// front, more than nine keep every octave's
	plan.emit = !plan.det_two || c->noct - 1 > 8 ? kEmitPerOctave : (c->noct <= 8 ? kEmitMultiAll : kEmitMultiRest);
}

static void plan_run(const sift3d_ctx *c, int upto, RunPlan &plan) {
	plan_small_launch(c, plan);
	plan_octaves(c, plan);
	plan_detect(c, upto, plan);
}

// One run = prepare (flags of the run) -> enqueue (the whole pipeline on the handle's streams, up to the asynchronous read-back of the
// five counters into pinned memory; no host synchronisation) -> finish (synchronise, check the list capacity, fill state and times;
// on overflow: regrow and enqueue again).  sift3d_run / sift3d_run_stages do all three; sift3d_run_async stops behind the first
// enqueue and sift3d_wait finishes (r04: one host thread keeps several handles in flight).
static int run_prepare(sift3d_ctx *c, int &upto) {
	if (c->slab) { set_last_error("a z-slab context is driven stage by stage (sift3d_slab_*)"); return SIFT3D_ERR_STATE; }
	if (c->pending) { set_last_error("the handle has an asynchronous run in flight: call sift3d_wait first"); return SIFT3D_ERR_STATE; }
	int rc = set_device(c->device);
	if (rc) return rc;
	if (upto < 1) upto = 1;
	if (upto > 5) upto = 5;
	// SIFT3D_HOOK_DOG_EAGER: write every DoG level
	const bool dog_eager = hook(SIFT3D_HOOK_DOG_EAGER) != 0;
	c->dog_elide = !dog_eager && c->nd >= 3;
	// the last Gaussian level is only ever read at the voxels that pass seven of the eight extremum tests of the last keypoint level:
	// it is not built at all; those voxels get the value from k_lazy_next (DetectLevels::lazy_src).  SIFT3D_HOOK_GLAST_EAGER builds it.
	const bool glast_eager = hook(SIFT3D_HOOK_GLAST_EAGER) != 0;
	c->g_last_elide = c->dog_elide && !glast_eager && c->use_fused && 2 * (2 * c->taps[c->ng - 1].hw + 1) <= kLazySlots;
	// detection options (sift3d_set_detect_options): the full neighbourhood and the fit read 3x3 blocks of DoG[0] and DoG[nd-1], so
	// such a run builds every level; a default handle keeps the elisions above unchanged
	c->run_full = c->dopt.neighbours == 80 || c->dopt.refine != 0;
	c->run_refine = c->dopt.refine != 0;
	if (c->run_full) { c->dog_elide = false; c->g_last_elide = false; }
	c->g_last_built.assign((size_t)std::max(1, c->noct), 0);
	c->n_regrow = 0;
	plan_run(c, upto, c->plan);
	return SIFT3D_OK;
}

static hipStream_t plan_stream(const sift3d_ctx *c, int index) { return index == kChainStream ? c->cstream : c->ostream[(size_t)index]; }

// a part of the pyramid that starts behind the seed level of `seed_octave`: the fork of the run first (the main stream reached the run)
static int wait_fork_and_seed(sift3d_ctx *c, hipStream_t so, int seed_octave) {
	S3D_HIP(hipStreamWaitEvent(so, c->ev_fork, 0));
	S3D_HIP(hipStreamWaitEvent(so, c->ev_seed[(size_t)seed_octave], 0));
	return SIFT3D_OK;
}

// level (0,0): the base blur of the input volume (a seeded context's was written by sift3d_seed_upload)
static void enqueue_base_blur(sift3d_ctx *c, const RunPlan &plan) {
	const RunPlan::Oct &oc = plan.oct[0];
	if (!c->seeded) smooth_level(c, 0, plan_stream(c, oc.head), oc.prio, oc.head_slots, c->in.d, c->gss[0], c->base_taps, nullptr, nullptr, nullptr);
}

// The head (levels up to the seed level G[o][num_kp_levels]) or the tail (the levels behind it) of octave o, with the events the
// other octaves and the detection wait for.  half_written[o]: level 0 of octave o was written by the seed level's kernel of octave o - 1
static int enqueue_octave_part(sift3d_ctx *c, const RunPlan &plan, int o, bool head, std::vector<char> &half_written) {
	const RunPlan::Oct &oc = plan.oct[(size_t)o];
	hipStream_t so = plan_stream(c, head ? oc.head : oc.tail);
	const int seed = c->p.num_kp_levels;
	int rc = SIFT3D_OK;
	if (head && o > 0 && (rc = wait_fork_and_seed(c, so, o - 1)) != SIFT3D_OK) return rc;
	if (plan.small_first >= 0 && o >= plan.small_first) {  // the whole octave is in the small launch, enqueued with the head of its first octave
		if (head && o == plan.small_first) {
			SmallArgs sa = plan.small;
			if (o == 0) enqueue_base_blur(c, plan);
			else if (!half_written[(size_t)o]) {  // the launch decimates the parent's seed level itself (no decimation launch)
				const Level &P = c->gss[(size_t)(o - 1) * c->ng + seed];
				sa.parent = P.d; sa.pnx = P.nx; sa.pny = P.ny;
			}
			launch_small_octaves(sa, so);
		}
		if (head) S3D_HIP(hipEventRecord(c->ev_seed[(size_t)o], so));
		if (!head && o > 0) S3D_HIP(hipEventRecord(c->ev_done[(size_t)o], so));
		return SIFT3D_OK;
	}
	// a tail on another stream than its head (chain stream, moved tail) follows the seed level by its event
	if (!head && o >= 1 && (plan.chain || oc.tail_moved) && (rc = wait_fork_and_seed(c, so, o)) != SIFT3D_OK) return rc;
	const int slots = head ? oc.head_slots : oc.tail_slots;
	for (int i = head ? 0 : seed + 1; i < (head ? seed + 1 : c->ng); i++) {
		const Level &L = c->gss[(size_t)o * c->ng + i];
		if (o == 0 && i == 0) enqueue_base_blur(c, plan);
		else if (i == 0) {
			const Level &P = c->gss[(size_t)(o - 1) * c->ng + seed];
			if (!half_written[(size_t)o]) launch_downsample(P.d, P.nx, P.ny, L.d, L.nx, L.ny, L.nz, so);
		} else {
			const Level &P = c->gss[(size_t)o * c->ng + i - 1];
			if (c->g_last_elide && i == c->ng - 1) continue;  // never built (k_lazy_next / sift3d_copy_level form what is asked for)
			// the seed level also leaves decimated, as level 0 of the next octave
			const Level *half = (i == seed && o + 1 < c->noct) ? &c->gss[(size_t)(o + 1) * c->ng] : nullptr;
			const bool elided = c->dog_elide && (i - 1 == 0 || i - 1 == c->nd - 1);  // a DoG level the pyramid does not write
			const bool hw = smooth_level(c, o, so, oc.prio, slots, P.d, L, c->taps[i], elided ? nullptr : P.d, elided ? nullptr : c->dog[(size_t)o * c->nd + i - 1].d,
			                             elided ? nullptr : c->d_dogmax + (size_t)o * c->nd + i - 1, half);
			if (half) half_written[(size_t)o + 1] = hw ? 1 : 0;
		}
		if (i == seed) S3D_HIP(hipEventRecord(c->ev_seed[(size_t)o], so));
	}
	if (!head && o > 0) S3D_HIP(hipEventRecord(c->ev_done[(size_t)o], so));
	return SIFT3D_OK;
}

// ---- Build_Gaussian_Scale_Space (Src/cSIFT3D.cc:268-319) with the DoG (346-360) fused into the z pass ----
// Every octave starts after the main stream reached this point (ev_fork); octave o is seeded by G[o-1][num_kp_levels] (DownSample_3D),
// everything else of octave o-1 overlaps with octave o.  Enqueue order: head(0), head(1), tail(0), head(2), tail(1), ...  The critical
// path of the stage is the chain of heads; the tail of octave 0 (its widest Gaussian) is machine-filling work off that path and starts
// together with head(1).
static int enqueue_pyramid(sift3d_ctx *c, const RunPlan &plan) {
	S3D_HIP(hipEventRecord(c->ev_fork, c->stream));
	std::vector<char> half_written((size_t)c->noct + 1, 0);
	int rc = SIFT3D_OK;
	for (int o = 0; o <= c->noct; o++) {
		if (o < c->noct && (rc = enqueue_octave_part(c, plan, o, true, half_written)) != SIFT3D_OK) return rc;
		if (o >= 1 && (rc = enqueue_octave_part(c, plan, o - 1, false, half_written)) != SIFT3D_OK) return rc;
	}
	return SIFT3D_OK;
}

// ---- the end of the pyramid stage and Detect_KeyPoints (Src/cSIFT3D.cc:362-425) ----
// With early masks octave 0's start right behind its last level, BESIDE the chains of the small octaves.  The pyramid stage still ends
// when EVERY octave's pyramid has: ev[1] is recorded on the second detection stream after it has waited for all of them, so the
// pyramid's time is its wall time and the detection's is what is left of it behind the pyramid.  ev[2]: the DoG is fused, a zero-length stage.
static int enqueue_detect(sift3d_ctx *c, const RunPlan &plan, int upto) {
	hipStream_t st = c->stream, sb = plan_stream(c, plan.det_two ? 1 : 0), sc = plan_stream(c, plan.det_rest_stream);
	std::vector<DetectLevels> DLs((size_t)c->noct);
	const int nl = c->nd - 2;  // DoG levels 1 .. nd-2 (Src/cSIFT3D.cc:376)
	const Taps *lt = c->g_last_elide ? &c->taps[c->ng - 1] : nullptr;
	DetectOpts dopt;
	dopt.neighbours = c->dopt.neighbours; dopt.refine = c->dopt.refine;
	dopt.max_offset = c->dopt.max_offset; dopt.contrast_thresh = c->dopt.contrast_thresh; dopt.edge_ratio = c->dopt.edge_ratio;
	const DetectOpts *dop = c->run_full ? &dopt : nullptr;  // null: the reference rule (k_mark)
	if (upto >= 3)
		for (int o = 0; o < c->noct; o++) fill_detect_levels(c, o, DLs[(size_t)o]);
	auto bufs = [&](int o) -> const DetectBufs & { return plan.det_two && o > 0 ? c->det_o[(size_t)o] : c->det; };
	auto mark = [&](int o, hipStream_t s) {
		const Level &C = c->dog[(size_t)o * c->nd + 1];
		launch_detect_mark(DLs[(size_t)o], nl, C.nx, C.ny, C.zr_all(), c->p.peak_thresh, o + c->octave_base, bufs(o), s, lt, dop);
	};
	hipStream_t join = plan.det_early ? sb : st;  // the stream that sees every octave's pyramid complete
	if (plan.det_early) {
		S3D_HIP(hipEventRecord(c->ev_det_fork, st));  // octave 0's pyramid is complete (the main stream is its stream)
		mark(0, st);
		S3D_HIP(hipStreamWaitEvent(sb, c->ev_det_fork, 0));
	}
	// (octave 1 too: its levels are in sb's own order only when neither the chain stream nor the small-octave launch took them)
	for (int o = 1; o < c->noct; o++) S3D_HIP(hipStreamWaitEvent(join, c->ev_done[(size_t)o], 0));
	S3D_HIP(hipEventRecord(c->ev[1], join));
	S3D_HIP(hipEventRecord(c->ev[2], join));
	if (upto < 3) return SIFT3D_OK;
	if (plan.det_two) {
		// the masks of the octaves >= 2 (launches of a few microseconds) beside octave 1's candidate pass; every octave has its own scratch
		for (int o = 1; o < c->noct; o++) {
			if (plan.det_rest_own && o >= 2) S3D_HIP(hipStreamWaitEvent(sc, c->ev_done[(size_t)o], 0));
			mark(o, o == 1 ? sb : sc);
		}
		S3D_HIP(hipEventRecord(c->ev_det_join, sb));
		if (sc != sb) S3D_HIP(hipEventRecord(c->ev_det_join2, sc));  // (the main stream waits for both itself: one hop across queues each, not two in a row)
	}
	std::vector<DetectEmitItem> multi;
	for (int o = 0; o < c->noct; o++) {
		const Level &C = c->dog[(size_t)o * c->nd + 1];
		if (!plan.det_two) mark(o, st);
		if (plan.det_two && o == 1) {
			S3D_HIP(hipStreamWaitEvent(st, c->ev_det_join, 0));
			if (sc != sb) S3D_HIP(hipStreamWaitEvent(st, c->ev_det_join2, 0));
		}
		if (plan.emit == kEmitMultiAll || (plan.emit == kEmitMultiRest && o > 0)) multi.push_back(DetectEmitItem{&DLs[(size_t)o], nl, C.nx, C.ny, C.zr_all(), o + c->octave_base, &bufs(o)});
		else launch_detect_emit(DLs[(size_t)o], nl, C.nx, C.ny, C.zr_all(), o + c->octave_base, bufs(o), c->d_ext, c->ext_cap, st);
	}
	if (!multi.empty()) launch_detect_emit_multi(multi.data(), (int)multi.size(), c->d_ext, c->ext_cap, c->d_total, st);
	return SIFT3D_OK;
}

// ---- Assign_Orientation (Src/cSIFT3D.cc:427-482) and Extract_Description (Src/cSIFT3D.cc:484-502) ----
void enqueue_slots(sift3d_ctx *c) {
	launch_slots(c->d_ext, c->d_codes, c->d_total, c->ext_cap, c->d_nkp, c->d_order, c->kp_cap, c->d_slots_part, c->stream);
}
void enqueue_orient(sift3d_ctx *c, int rank, int world) {
	launch_orient(c->d_ext, c->d_codes, c->d_total, c->ext_cap, c->d_levels, c->d_luts, c->d_lutpool, c->p.max_eig_thres, c->p.corner_thresh,
	              rank, world, c->d_order, c->d_nkp + 3, c->stream);
	enqueue_slots(c);
}
void enqueue_describe(sift3d_ctx *c, int rank, int world, bool with_desc) {
	if (with_desc)
		launch_describe(c->d_ext, c->d_total, c->ext_cap, c->d_levels, c->d_luts, c->d_lutpool, c->d_desc, c->kp_cap, rank, world, c->d_order,
		                c->d_nkp, c->d_nkp + 1, c->stream, c->desc_lut_lds, &c->dsplit);
	launch_finalize(c->d_ext, c->d_total, c->ext_cap, with_desc, c->d_kpout, c->d_xyz, c->kp_cap, c->stream);
}

// scratch of a run that the lists' capacity or an earlier error decides
static int run_scratch(sift3d_ctx *c, int upto) {
	if (c->run_refine && upto >= 4 && c->refined_cap < c->kp_cap) {  // (first refining run, or the lists were regrown)
		hipFree(c->d_refined); c->d_refined = nullptr; c->refined_cap = 0;
		S3D_HIP(hipMalloc(&c->d_refined, sizeof(sift3d_refined) * (size_t)c->kp_cap));
		c->refined_cap = c->kp_cap;
	}
	if (c->dsplit_dirty && c->dsplit.gacc) {  // (a run cut short by an error may have left partial sums / arrival counts behind)
		S3D_HIP(hipMemsetAsync(c->dsplit.gacc, 0, sizeof(int) * (size_t)c->dsplit.cap * (kDesc + 8 + 1), c->stream));
		c->dsplit_dirty = false;
	}
	return SIFT3D_OK;
}

// the stages of c->plan, one after the other, between the events that time them (ev[1] and ev[2]: enqueue_detect)
static int run_enqueue(sift3d_ctx *c, int upto, bool part_orient) {
	int rc = set_device(c->device);
	if (rc) return rc;
	if ((rc = run_scratch(c, upto)) != SIFT3D_OK) return rc;
	hipStream_t st = c->stream;
	const RunPlan &plan = c->plan;
	if (c->gate) { S3D_HIP(hipStreamWaitEvent(st, c->gate, 0)); c->gate = nullptr; }
	S3D_HIP(hipMemsetAsync(c->d_dogmax, 0, sizeof(unsigned) * (size_t)(std::max(1, c->noct * c->nd) + 6), st));
	S3D_HIP(hipEventRecord(c->ev[0], st));
	if ((rc = enqueue_pyramid(c, plan)) != SIFT3D_OK) return rc;
	if ((rc = enqueue_detect(c, plan, upto)) != SIFT3D_OK) return rc;
	S3D_HIP(hipEventRecord(c->ev[3], st));
	if (upto >= 4) enqueue_orient(c, part_orient ? c->part_rank : 0, part_orient ? c->part_world : 1);
	S3D_HIP(hipEventRecord(c->ev[4], st));
	if (upto >= 4) enqueue_describe(c, c->part_rank, c->part_world, upto >= 5);
	if (upto >= 4 && c->run_refine) {  // refined records of the accepted keypoints (timed with the descriptor stage)
		DogTable T;
		fill_dog_table(c, T);
		launch_refine(c->d_ext, c->d_total, c->ext_cap, c->kp_cap, T, c->p.num_kp_levels, c->d_refined, st);
	}
	S3D_HIP(hipEventRecord(c->ev[5], st));
	// total, overflow, nkp, describe work counter, describe second passes -> pinned host words
	S3D_HIP(hipMemcpyAsync(c->h_words, c->d_total, sizeof(unsigned) * 5, hipMemcpyDeviceToHost, st));
	return SIFT3D_OK;
}


// synchronise with the enqueued run and take its results; again = the lists overflowed and were regrown: enqueue once more
static int run_finish(sift3d_ctx *c, int upto, bool &again) {
	again = false;
	int rc = set_device(c->device);
	if (rc) return rc;
	hipStream_t st = c->stream;
	{
		unsigned *host_words = c->h_words;
		S3D_HIP(hipStreamSynchronize(st));
		S3D_HIP(hipGetLastError());
		if (host_words[1] != 0 || host_words[0] > c->ext_cap) {
			// list overflow: regrow to fit and rerun (rare; sizes are generous).  The detection kernels keep counting past the
			// capacity, so host_words[0] is the number of extrema of the volume (short of candidates dropped from a full parking list).
			const unsigned need = std::max(host_words[0], c->ext_cap) * 2u;
			rc = alloc_lists(c, need);
			if (rc) return rc;
			c->n_regrow++;
			again = true;
			return SIFT3D_OK;
		}
		c->n_ext = host_words[0];
		c->n_kp = upto >= 4 ? host_words[2] : 0;
		c->n_desc_redo = upto >= 5 ? (int)host_words[4] : 0;
		c->stage = upto;
		c->last_refine = c->run_refine && upto >= 4;
		float ms = 0;
		auto dt = [&](int a, int b) { hipEventElapsedTime(&ms, c->ev[a], c->ev[b]); return (double)ms * 1e-3; };
		c->times[0] = dt(0, 5); c->times[1] = 0; c->times[2] = dt(0, 1); c->times[3] = dt(1, 2);
		c->times[4] = dt(2, 3); c->times[5] = dt(3, 4); c->times[6] = dt(4, 5); c->times[7] = 0;
		return SIFT3D_OK;
	}
}

static int run_complete(sift3d_ctx *c, int upto, bool part_orient) {  // behind an enqueue: finish, re-enqueueing while the lists overflow
	for (int attempt = 0; attempt < 8; attempt++) {
		bool again = false;
		int rc = run_finish(c, upto, again);
		if (rc) return rc;
		if (!again) return SIFT3D_OK;
		if ((rc = run_enqueue(c, upto, part_orient)) != SIFT3D_OK) return rc;
	}
	(void)hipStreamSynchronize(c->stream);
	set_last_error("extrema list kept overflowing");
	return SIFT3D_ERR_CAPACITY;
}

int run_impl(sift3d_ctx *c, int upto, bool part_orient) {
	int rc = run_prepare(c, upto);
	if (rc) return rc;
	if ((rc = run_enqueue(c, upto, part_orient)) == SIFT3D_OK) rc = run_complete(c, upto, part_orient);
	if (rc) c->dsplit_dirty = true;
	return rc;
}

extern "C" int sift3d_run(sift3d_handle c) {
	if (!c) return SIFT3D_ERR_ARG;
	return run_impl(c, 5);
}

// KpSiftAlgorithm without the wait: the whole pipeline is enqueued on the handle's own streams and the call returns; sift3d_wait
// completes it.  One host thread can so keep several handles (volumes) in flight on one GPU -- the pyramid of one volume is bound by
// memory, the descriptors of another by instruction issue (BASELINE configs[2] / [4]: several volumes per GPU).
extern "C" int sift3d_run_async(sift3d_handle c) {
	if (!c) return SIFT3D_ERR_ARG;
	int upto = 5;
	int rc = run_prepare(c, upto);
	if (rc) return rc;
	if ((rc = run_enqueue(c, upto, false)) != SIFT3D_OK) { (void)hipStreamSynchronize(c->stream); c->dsplit_dirty = true; return rc; }
	c->pending = true;
	return SIFT3D_OK;
}

// Two volumes back to back on one GPU (Example.cpp:21-44 extracts a reference and a target volume one after the other): the second
// volume's pipeline starts when the FIRST volume's orientation stage has ended, i.e. its memory-bound front (pyramid, extrema, orientation)
// runs beside the first volume's descriptor stage, which is bound by instruction issue and the LDS.  `after` must have a run in flight
// (sift3d_run_async) on the same device; otherwise this is sift3d_run_async.
extern "C" int sift3d_run_async_after(sift3d_handle c, sift3d_handle after) {
	if (!c) return SIFT3D_ERR_ARG;
	if (after && after != c && after->pending && after->device == c->device) c->gate = after->ev[4];
	const int rc = sift3d_run_async(c);
	c->gate = nullptr;
	return rc;
}

extern "C" int sift3d_wait(sift3d_handle c) {
	if (!c) return SIFT3D_ERR_ARG;
	if (!c->pending) return SIFT3D_OK;  // nothing in flight (a blocking run has completed already)
	c->pending = false;
	const int rc = run_complete(c, 5, false);
	if (rc) c->dsplit_dirty = true;
	return rc;
}

extern "C" int sift3d_run_stages(sift3d_handle c, int upto) {
	if (!c) return SIFT3D_ERR_ARG;
	return run_impl(c, upto);
}

extern "C" int sift3d_stage_times(sift3d_handle c, double t[8]) {
	if (!c || !t) return SIFT3D_ERR_ARG;
	if (c->pending) { int wrc = sift3d_wait(c); if (wrc) return wrc; }  // an asynchronous run in flight is completed first
	if (c->stage < 1) return SIFT3D_ERR_STATE;
	memcpy(t, c->times, sizeof(double) * 8);
	return SIFT3D_OK;
}

extern "C" int sift3d_num_keypoints(sift3d_handle c, int *n) {
	if (!c || !n) return SIFT3D_ERR_ARG;
	if (c->pending) { int wrc = sift3d_wait(c); if (wrc) return wrc; }  // an asynchronous run in flight is completed first
	*n = (c->stage >= 4) ? (int)c->n_kp : 0;  // GetKeypoints before KpSiftAlgorithm returns empty
	return SIFT3D_OK;
}

extern "C" int sift3d_get_keypoints(sift3d_handle c, sift3d_keypoint *out, float *desc) {
	if (!c) return SIFT3D_ERR_ARG;
	if (c->pending) { int wrc = sift3d_wait(c); if (wrc) return wrc; }  // an asynchronous run in flight is completed first
	if (c->stage < 4 || c->n_kp == 0) return SIFT3D_OK;
	int rc = set_device(c->device);
	if (rc) return rc;
	if (desc && c->stage < 5) return SIFT3D_ERR_STATE;
	// results were complete when the run returned; the copies go through the pinned staging pool on the handle's own stream
	D2HSeg sg[2];
	int ns = 0;
	if (out) sg[ns++] = D2HSeg{out, c->d_kpout, sizeof(sift3d_keypoint) * (size_t)c->n_kp};
	if (desc) sg[ns++] = D2HSeg{desc, c->d_desc, sizeof(float) * kDesc * (size_t)c->n_kp};
	return staged_d2h_v(sg, ns, c->device, c->own_stream);
}

extern "C" int sift3d_device_results(sift3d_handle c, const float **d_desc, const float **d_xyz, int *n) {
	if (!c) return SIFT3D_ERR_ARG;
	if (c->pending) { int wrc = sift3d_wait(c); if (wrc) return wrc; }  // an asynchronous run in flight is completed first
	if (c->stage < 5) return SIFT3D_ERR_STATE;
	if (d_desc) *d_desc = c->d_desc;
	if (d_xyz) *d_xyz = c->d_xyz;
	if (n) *n = (int)c->n_kp;
	return SIFT3D_OK;
}

extern "C" int sift3d_match_handles(sift3d_handle ref, sift3d_handle tar, double thresHold, int mode, int *gIdx, int *sIdx, float *gDist,
                                    float *sDist, float *pairs6, int *npairs, double *seconds) {
	if (!ref || !tar) return SIFT3D_ERR_ARG;
	int rc;
	if (ref->pending && (rc = sift3d_wait(ref)) != SIFT3D_OK) return rc;
	if (tar->pending && (rc = sift3d_wait(tar)) != SIFT3D_OK) return rc;
	if (ref->stage < 5 || tar->stage < 5) { set_last_error("sift3d_match_handles: both extractors must have run"); return SIFT3D_ERR_STATE; }
	const int n = (int)ref->n_kp, m = (int)tar->n_kp;
	const float *td = tar->d_desc, *tx = tar->d_xyz;
	if ((tar->device != ref->device || hook(SIFT3D_HOOK_PEER_COPY)) && m > 0) {
		// the target's results live on another GPU: one peer-to-peer copy (xGMI) into a scratch on the reference's device
		if ((rc = set_device(ref->device)) != SIFT3D_OK) return rc;
		const size_t need = (size_t)m * (kDesc + 3);
		if (need > ref->peer_floats) {
			if (ref->d_peer) (void)hipFree(ref->d_peer);
			ref->d_peer = nullptr; ref->peer_floats = 0;
			S3D_HIP(hipMalloc(&ref->d_peer, sizeof(float) * (need + need / 4)));
			ref->peer_floats = need + need / 4;
		}
		S3D_HIP(hipMemcpyPeer(ref->d_peer, ref->device, tar->d_desc, tar->device, sizeof(float) * (size_t)m * kDesc));
		S3D_HIP(hipMemcpyPeer(ref->d_peer + (size_t)m * kDesc, ref->device, tar->d_xyz, tar->device, sizeof(float) * (size_t)m * 3));
		td = ref->d_peer; tx = ref->d_peer + (size_t)m * kDesc;
	}
	return sift3d_match(ref->d_desc, ref->d_xyz, n, td, tx, m, thresHold, mode, 1, ref->device, gIdx, sIdx, gDist, sDist, pairs6, npairs, seconds);
}

// No reference counterpart (generalises IsExtrema_neighbor, Src/cSIFT3D.cc:884-911): see include/sift3d_hip.h
extern "C" int sift3d_set_detect_options(sift3d_handle c, const sift3d_detect_options *o) {
	if (!c || !o) { set_last_error("sift3d_set_detect_options: null argument"); return SIFT3D_ERR_ARG; }
	if (c->slab || c->seeded) { set_last_error("sift3d_set_detect_options: only plain single-volume handles (sift3d_create) take detection options"); return SIFT3D_ERR_ARG; }
	if (c->pending) { set_last_error("sift3d_set_detect_options: the handle has an asynchronous run in flight: call sift3d_wait first"); return SIFT3D_ERR_STATE; }
	if (o->neighbours != 8 && o->neighbours != 80) { set_last_error("sift3d_set_detect_options: neighbours must be 8 or 80"); return SIFT3D_ERR_ARG; }
	if (o->refine != 0 && o->refine != 1) { set_last_error("sift3d_set_detect_options: refine must be 0 or 1"); return SIFT3D_ERR_ARG; }
	if (!isfinite(o->max_offset) || !isfinite(o->contrast_thresh) || !isfinite(o->edge_ratio)) {
		set_last_error("sift3d_set_detect_options: thresholds must be finite");
		return SIFT3D_ERR_ARG;
	}
	if (o->reserved[0] || o->reserved[1] || o->reserved[2]) { set_last_error("sift3d_set_detect_options: reserved words must be 0"); return SIFT3D_ERR_ARG; }
	if (c->noct > kDogTabOct || c->nd > kDogTabLv) { set_last_error("sift3d_set_detect_options: too many octaves / levels for the refinement table"); return SIFT3D_ERR_ARG; }
	c->dopt = *o;
	return SIFT3D_OK;
}

// No reference counterpart (generalises Src/cSIFT3D.cc:884-911)
extern "C" int sift3d_get_detect_options(sift3d_handle c, sift3d_detect_options *o) {
	if (!c || !o) return SIFT3D_ERR_ARG;
	*o = c->dopt;
	return SIFT3D_OK;
}

// No reference counterpart (generalises Src/cSIFT3D.cc:884-911): the refined records of the last completed run, slot order
extern "C" int sift3d_get_refined(sift3d_handle c, sift3d_refined *out) {
	if (!c || !out) return SIFT3D_ERR_ARG;
	if (c->pending) { int wrc = sift3d_wait(c); if (wrc) return wrc; }  // an asynchronous run in flight is completed first
	if (!c->last_refine || c->stage < 4) { set_last_error("sift3d_get_refined: the last completed run did not refine its keypoints"); return SIFT3D_ERR_STATE; }
	if (c->n_kp == 0) return SIFT3D_OK;
	int rc = set_device(c->device);
	if (rc) return rc;
	return staged_d2h(out, c->d_refined, sizeof(sift3d_refined) * (size_t)c->n_kp, c->device, c->own_stream);
}

extern "C" int sift3d_num_octaves(sift3d_handle c, int *n) {
	if (!c || !n) return SIFT3D_ERR_ARG;
	*n = c->noct;
	return SIFT3D_OK;
}

static const Level *pick_level(sift3d_ctx *c, int is_dog, int idx) {
	const std::vector<Level> &P = is_dog ? c->dog : c->gss;
	if (idx < 0 || (size_t)idx >= P.size()) return nullptr;
	return &P[idx];
}

extern "C" int sift3d_level_info(sift3d_handle c, int is_dog, int idx, int dims3[3], float units3[3], float *scale) {
	if (!c) return SIFT3D_ERR_ARG;
	const Level *L = pick_level(c, is_dog, idx);
	if (!L) return SIFT3D_ERR_ARG;
	if (dims3) { dims3[0] = L->nx; dims3[1] = L->ny; dims3[2] = L->nz; }
	if (units3) units3[0] = units3[1] = units3[2] = L->unit;
	if (scale) *scale = L->scale;
	return SIFT3D_OK;
}

extern "C" int sift3d_copy_level(sift3d_handle c, int is_dog, int idx, float *out) {
	if (!c || !out) return SIFT3D_ERR_ARG;
	if (c->pending) { int wrc = sift3d_wait(c); if (wrc) return wrc; }  // an asynchronous run in flight is completed first
	if (c->stage < 1) return SIFT3D_ERR_STATE;
	const Level *L = pick_level(c, is_dog, idx);
	if (!L) return SIFT3D_ERR_ARG;
	int rc = set_device(c->device);
	if (rc) return rc;
	if (c->g_last_elide && c->slab) {
		// z-slab context: build the owned planes of the last Gaussian level on request (G[nd-1] holds its halo)
		const int i = is_dog ? idx % c->nd : idx % c->ng;
		if (((is_dog && i == c->nd - 1) || (!is_dog && i == c->ng - 1)) && (c->g_last_built.empty() || !c->g_last_built[0])) {
			const Level &G = c->gss[c->ng - 1];
			if (!launch_march_level(c->gss[c->ng - 2].d, G.d, nullptr, nullptr, G.nx, G.ny, G.zr(c->own0 - G.zoff, c->own1 - G.zoff), c->taps[c->ng - 1],
			                        c->stream)) return SIFT3D_ERR_STATE;
			S3D_HIP(hipStreamSynchronize(c->stream));
			c->g_last_built.assign(1, 1);
		}
	}
	if (c->g_last_elide && !c->slab) {
		// the last Gaussian level of the octave (and the DoG level behind it) was never built: build it now, once
		const int o = is_dog ? idx / c->nd : idx / c->ng, i = is_dog ? idx % c->nd : idx % c->ng;
		if (((is_dog && i == c->nd - 1) || (!is_dog && i == c->ng - 1)) && !c->g_last_built[(size_t)o]) {
			const Level &G = c->gss[(size_t)o * c->ng + c->ng - 1], &P = c->gss[(size_t)o * c->ng + c->ng - 2];
			const RunPlan::Oct &oc = c->plan.oct[(size_t)o];  // (launched as the run would have launched it)
			smooth_level(c, o, c->ostream[o], oc.prio, oc.tail_slots, P.d, G, c->taps[c->ng - 1], nullptr, nullptr, nullptr);
			S3D_HIP(hipStreamSynchronize(c->ostream[o]));
			c->g_last_built[(size_t)o] = 1;
		}
	}
	if (is_dog && c->dog_elide && (idx % c->nd == 0 || idx % c->nd == c->nd - 1)) {
		// an elided DoG level (never written by the pipeline): form it now, exactly like Sub, into its arena slot
		const int o = idx / c->nd, i = idx % c->nd;
		launch_dog_from_gss(c->gss[(size_t)o * c->ng + i + 1].d, c->gss[(size_t)o * c->ng + i].d, L->d, L->n(), c->stream);
		S3D_HIP(hipStreamSynchronize(c->stream));
	}
	return staged_d2h(out, L->d, sizeof(float) * L->n(), c->device, c->own_stream);
}

extern "C" int sift3d_copy_input(sift3d_handle c, float *out) {
	if (!c || !out) return SIFT3D_ERR_ARG;
	int rc = set_device(c->device);
	if (rc) return rc;
	return staged_d2h(out, c->in.d, sizeof(float) * c->in.n(), c->device, c->own_stream);
}

extern "C" int sift3d_num_extrema(sift3d_handle c, int *n) {
	if (!c || !n) return SIFT3D_ERR_ARG;
	if (c->pending) { int wrc = sift3d_wait(c); if (wrc) return wrc; }  // an asynchronous run in flight is completed first
	*n = c->stage >= 3 ? (int)c->n_ext : 0;
	return SIFT3D_OK;
}

static int fetch_ext(sift3d_ctx *c, std::vector<DevKp> &h) {
	int rc = set_device(c->device);
	if (rc) return rc;
	h.resize(c->n_ext);
	if (c->n_ext) S3D_HIP(hipMemcpy(h.data(), c->d_ext, sizeof(DevKp) * (size_t)c->n_ext, hipMemcpyDeviceToHost));
	return SIFT3D_OK;
}

extern "C" int sift3d_get_extrema(sift3d_handle c, sift3d_keypoint *out) {
	if (!c || !out) return SIFT3D_ERR_ARG;
	if (c->pending) { int wrc = sift3d_wait(c); if (wrc) return wrc; }  // an asynchronous run in flight is completed first
	if (c->stage < 3) return SIFT3D_ERR_STATE;
	std::vector<DevKp> h;
	int rc = fetch_ext(c, h);
	if (rc) return rc;
	for (size_t i = 0; i < h.size(); i++) {
		sift3d_keypoint &o = out[i];
		memset(&o, 0, sizeof(o));
		o.x = (float)h[i].x; o.y = (float)h[i].y; o.z = (float)h[i].z;
		o.scale = h[i].scale; o.octave = h[i].octave; o.level = h[i].level;
		o.rx = o.ry = o.rz = -1.0f;
		memcpy(o.win, h[i].win, sizeof(o.win));
		memcpy(o.eigvalue, h[i].eigvalue, sizeof(o.eigvalue));
		memcpy(o.eigvector, h[i].eigvector, sizeof(o.eigvector));
		memcpy(o.Rotation, h[i].rot, sizeof(o.Rotation));
		memcpy(o.str_tensor, h[i].st, sizeof(o.str_tensor));
	}
	return SIFT3D_OK;
}

extern "C" int sift3d_get_orientation_codes(sift3d_handle c, int *codes) {
	if (!c || !codes) return SIFT3D_ERR_ARG;
	if (c->pending) { int wrc = sift3d_wait(c); if (wrc) return wrc; }  // an asynchronous run in flight is completed first
	if (c->stage < 4) return SIFT3D_ERR_STATE;
	std::vector<DevKp> h;
	int rc = fetch_ext(c, h);
	if (rc) return rc;
	for (size_t i = 0; i < h.size(); i++) codes[i] = h[i].code;
	return SIFT3D_OK;
}

}  // namespace s3d
