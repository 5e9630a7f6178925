// ctx_internal.h -- the context of the HIP library and the host helpers its translation units share (not part of the C-ABI).
//   context.hip     life cycle of a sift3d_ctx, the KpSiftAlgorithm pipeline (Src/cSIFT3D.cc:165-235) and its accessors
//   tables.hip      host-built constants: Gaussian taps, icosahedron faces + symmetry table, window weight tables
//   entry_free.hip  the reference's free functions on caller-held host data (Include/cSIFT3D.h:208-239)
//   entry_slab.hip  seeded contexts and z-slab contexts of the multi-GPU sharding
//   entry_test.hip  test hooks, rare-path counters, unit-level debug entry points (include/sift3d_hip_test.h)
#pragma once

#include <string>
#include <thread>
#include <vector>

#include "sift3d_internal.h"

// (the context is the C-ABI's opaque `struct sift3d_ctx`: global scope; its members are the library's types)
using s3d::DescSplit; using s3d::DetectBufs; using s3d::DevKp; using s3d::Level; using s3d::LevelRef; using s3d::Taps; using s3d::WinLut;


// ---------------------------------------------------------------------------------------------
// The schedule of a whole-volume run as data ("The schedule of a run"): plan_run decides, once per run, from the geometry,
// the flags of the run (sift3d_ctx::dog_elide, g_last_elide, run_full: not repeated here) and the streams the context owns; the
// enqueue_* functions of context.hip only walk it.  Plain values and indices, no handles.  A stream index is an octave's
// (sift3d_ctx::ostream) or kChainStream (sift3d_ctx::cstream).
// ---------------------------------------------------------------------------------------------
constexpr int kChainStream = -1;
enum { kEmitPerOctave = 0, kEmitMultiRest = 1, kEmitMultiAll = 2 };
struct RunPlan {
	// head = the levels of an octave up to its seed level G[o][num_kp_levels], tail = the levels behind it
	struct Oct {
		int head = 0, tail = 0;         // stream index of either part
		bool tail_moved = false;        // the tail runs on the stream of the octave above
		int prio = 0;                   // wave priority of the octave's launches
		int head_slots = 0, tail_slots = 0;  // slot plan of its levels (0: the launch's own)
	};
	std::vector<Oct> oct;
	bool chain = false;               // the chain stream exists: heads of the octaves >= 1 and the small launch run on it
	int small_first = -1;             // first octave of the small-octave launch (every octave behind it is in it too); -1: none
	s3d::SmallArgs small{};           // its arguments, short of `parent` (known when the seed level above has been enqueued)
	// detection
	bool det_two = false;             // octaves >= 1 form their masks in the second scratch, on octave 1's stream
	bool det_early = false;           // octave 0's masks start behind octave 0's pyramid, not behind every octave's
	int det_rest_stream = 0;          // stream index of the masks of the octaves >= 2
	bool det_rest_own = false;        // ... each behind its own pyramid (ev_done) instead of behind all of them
	int emit = kEmitPerOctave;        // how the ordered compaction is launched: per octave, one launch for the octaves >= 1, one for all
};

// ---------------------------------------------------------------------------------------------
// the context
// ---------------------------------------------------------------------------------------------
struct sift3d_ctx {
	int device = 0;
	hipStream_t stream = nullptr;
	hipStream_t own_stream = nullptr;  // the stream this context created (stream may be replaced by sift3d_set_stream)
	sift3d_params p{};
	int nx = 0, ny = 0, nz = 0;     // dims of the first octave this context holds (global)
	int noct = 0, ng = 0, nd = 0;
	int octave_base = 0;            // absolute index of that octave (seeded contexts of the multi-GPU path start at 1)
	bool seeded = false;            // level (0,0) is written by the caller (sift3d_seed_upload); no input volume, no base blur
	// z-slab mode (multi-GPU sharding of octave 0): this context owns global planes [own0, own1) and every level buffer
	// holds planes [own0-halo, own1+halo); halo planes are filled by the caller (neighbour exchange)
	bool slab = false;
	int own0 = 0, own1 = 0, halo = 0;
	// single-volume path: DoG[o][0] and DoG[o][nd-1] are not written by the pyramid (see DetectLevels); copy_level forms them
	bool dog_elide = false;
	bool g_last_elide = false;      // the last Gaussian level of every octave is not built (DetectLevels::lazy_src); implies dog_elide
	std::vector<char> g_last_built; // per octave: built on request (sift3d_copy_level)
	unsigned *d_prov = nullptr;     // parked candidates of the lazy level + [prov_cap] = their count
	bool desc_lut_lds = true;       // every descriptor window weight table fits the LDS copy (kMaxDescLut)
	bool ext_arena = false;         // level buffers live in memory owned by the caller
	int part_rank = 0, part_world = 1;  // descriptor work split of replicated octaves

	// device memory
	float *arena = nullptr;       // input + pyramids + scratch (one allocation)
	// r05: a HOST volume gets its own input buffer, allocated first, and a thread that stages the volume into it (staging.hip) while the
	// constructor allocates everything else (the 8 GB arena, the lists, the tables: 4 ms that used to come in front of the 10 ms copy)
	float *in_own = nullptr;
	void *in_raw = nullptr;       // sift3d_create_typed, host volume: the integer voxels as uploaded; freed before that call returns
	hipStream_t up_stream = nullptr;
	std::thread uploader;
	int upload_rc = SIFT3D_OK;
	std::string upload_err;
	size_t arena_floats = 0;
	Level in;
	std::vector<Level> gss, dog;
	std::vector<float *> tmpA, tmpB;        // per-octave scratch of the generic separable passes (octaves may overlap)
	// one stream per octave (ostream[0] == stream) and, for volumes of at most 4 M voxels, one chain stream for the heads of the
	// octaves >= 1 (nullptr otherwise).  Which part of which octave runs where is the RunPlan's business: DESIGN.md, "The schedule of a run"
	std::vector<hipStream_t> ostream;
	hipStream_t cstream = nullptr;
	std::vector<hipEvent_t> ev_seed, ev_done;
	hipEvent_t ev_fork = nullptr;
	unsigned *d_words = nullptr;  // [0] input max bits, [1..] per-DoG-level max bits, then counters
	unsigned *d_slots_part = nullptr;  // scratch of launch_slots (per-wave totals)
	unsigned *h_words = nullptr;  // pinned: the five counters a run reads back (a pageable destination makes the copy a staged, synchronous one)
	unsigned *d_inmax = nullptr, *d_dogmax = nullptr, *d_total = nullptr, *d_nkp = nullptr;
	DetectBufs det{};
	size_t det_blocks = 0;
	// octaves >= 1 own a slice of a second detection scratch: their masks are formed on a second stream beside octave 0's, only
	// the ordered compaction into the extrema list stays serial (S3D_DET_SERIAL=1: everything on one stream, one scratch)
	std::vector<DetectBufs> det_o;
	unsigned long long *d_masks2 = nullptr;
	unsigned *d_counts2 = nullptr, *d_offsets2 = nullptr, *d_prov2 = nullptr;
	hipEvent_t ev_det_fork = nullptr, ev_det_join = nullptr, ev_det_join2 = nullptr;
	DevKp *d_ext = nullptr;
	int *d_codes = nullptr, *d_order = nullptr;  // d_order: slot -> extremum index
	unsigned ext_cap = 0, kp_cap = 0;
	LevelRef *d_levels = nullptr;
	WinLut *d_luts = nullptr;
	float *d_lutpool = nullptr;
	sift3d_keypoint *d_kpout = nullptr;
	float *d_desc = nullptr, *d_xyz = nullptr;
	DescSplit dsplit{};             // scratch of the split descriptor windows (runs with few keypoints), one allocation at dsplit.gacc
	bool ghost = false;             // slab contexts (r06): every level is produced on ghost planes beyond the owned range too (sift3d_slab_set_ghost): no per-level halo exchange
	bool desc_partial = false;      // slab contexts (r05): descriptor windows are split along z over the ranks -- the halo of G[1..levels] only has to carry the orientation windows
	bool dsplit_dirty = false;      // a run ended in an error: the "every run leaves the scratch clean" invariant is re-established by the next run
	float *d_peer = nullptr;        // sift3d_match_handles: a target's descriptors + coordinates copied from another GPU (grow-only)
	size_t peer_floats = 0;

	// host tables
	std::vector<Taps> taps;  // per GSS level index within an octave
	Taps base_taps{};

	// sift3d_set_detect_options (plain contexts only): dopt = the options of the next run; run_opts = those of the run enqueued last
	// (set by run_prepare: a non-default run materialises every DoG level and the last Gaussian level); last_refine = the last
	// COMPLETED run refined its keypoints (d_refined holds n_kp records, sized kp_cap and reallocated behind a list regrow)
	sift3d_detect_options dopt{};
	bool run_full = false, run_refine = false, last_refine = false;
	RunPlan plan;  // the schedule of the run prepared last (run_prepare); a list regrow enqueues the same plan again
	sift3d_refined *d_refined = nullptr;
	unsigned refined_cap = 0;

	bool nonfinite = false;  // the input volume holds a NaN or Inf (k_absmax's flag, read once in sift3d_create): every level by k_conv_axis's `exact` form
	bool use_fused = true;  // SIFT3D_HOOK_SEPARABLE forces the generic three-pass kernels (parity cross-check)
	int n_regrow = 0, n_desc_redo = 0;  // sift3d_debug_counters: list regrows / second descriptor passes of the last run

	// results / state
	int stage = 0;  // highest stage run
	bool pending = false;  // sift3d_run_async enqueued a run that sift3d_wait has not completed yet
	hipEvent_t gate = nullptr;  // sift3d_run_async_after: the next enqueue starts behind this event (another handle's orientation stage); one shot
	unsigned n_ext = 0, n_kp = 0;
	hipEvent_t ev[8] = {};
	double times[8] = {};
};

// how a context is built: the classic whole-volume extractor, a SEEDED tail (octaves >= octave_base starting from a
// caller-provided G[octave_base][0]) or a z-SLAB of octave 0 (multi-GPU sharding)
struct CreateCfg {
	int nx = 0, ny = 0, nz = 0;   // global dims of the first octave held
	int octave_base = 0;
	int noct_total = -1;          // octaves counted on the ORIGINAL volume (Src/cSIFT3D.cc:254-255); -1: from nx,ny,nz
	bool seeded = false;
	bool slab = false;
	int z0 = 0, z1 = 0, halo = 0;
	const void *host_volume = nullptr;   // plain extractor on a pageable host volume: uploaded beside the allocations (sift3d_ctx::uploader)
	int host_dtype = SIFT3D_DT_F32;      // its voxels: fp32 lands in the input buffer, an integer type (sift3d_create_typed) in sift3d_ctx::in_raw
	float *ext_arena = nullptr;   // slab: caller-owned device memory for the level buffers (so that the caller's
	size_t ext_arena_floats = 0;  // communication layer can address halo planes directly), see sift3d_slab_arena_floats
};

namespace s3d {
// tables.hip
bool build_taps(float sigma, Taps &t);
void level_sigmas(const sift3d_params &p, std::vector<float> &sig, float &base_sigma);
void build_faces(FaceConst *F);
bool build_facesym(const FaceConst *F, FaceSym *S);
bool append_lut(std::vector<float> &pool, WinLut &L, int which, float sigma, float radius, float u, float scale);
// context.hip
int set_device(int device);
int alloc_lists(sift3d_ctx *c, unsigned ext_cap);
float level_scale(const sift3d_params &p, int octave, int s);  // scale of level s of the ABSOLUTE octave (Src/cUtil.cc:215-225)
void plan_pyramid(sift3d_ctx *c, int noct_total);
void fill_detect_levels(const sift3d_ctx *c, int o, DetectLevels &DL);
// Assign_Orientation + the slots of the accepted keypoints, Extract_Description (with_desc) + the final records, on the context's
// stream: the whole-volume run, the replicated octaves (sift3d_run_describe) and the slab stages share them
void enqueue_slots(sift3d_ctx *c);
void enqueue_orient(sift3d_ctx *c, int rank, int world);
void enqueue_describe(sift3d_ctx *c, int rank, int world, bool with_desc);
int upload_luts(sift3d_ctx *c, const std::vector<WinLut> &luts, std::vector<float> &pool);
std::vector<WinLut> blank_luts(const sift3d_ctx *c);
size_t arena_floats_of(const sift3d_ctx *c);
int create_common(sift3d_handle *out, const CreateCfg &cfg, const sift3d_params *params, int device);
int join_upload(sift3d_ctx *c);  // the uploader thread has ended and every chunk has landed; its error (and text) otherwise
int run_impl(sift3d_ctx *c, int upto, bool part_orient = false);
}  // namespace s3d
