/*
 * sift3d_hip.h -- C-ABI of the MI355X-native 3D SIFT library (lib: 3dsift_amd/libsift3d_hip.so).
 *
 * This is the drop-in boundary: plain C types, opaque handle, int error codes, no exceptions, no
 * torch types.  The C++ shell in 3dsift_amd/host/ (namespace CPUSIFT, same class / method names as
 * the reference) and the python ctypes binding in 3dsift_amd/capi.py are both thin layers over
 * exactly these entry points.  Each entry point cites the reference interface it replaces
 * (paths relative to the reference repo, 3DSIFT/...).
 *
 * Pointers are HOST pointers unless the name says otherwise (d_ prefix / "device" flag).
 * All volumes are fp32, x fastest: idx = x + nx*(y + ny*z)   (Include/Util/cTexImage.h:5,35).
 * A handle serialises its calls on one HIP stream; different handles are independent.
 */
#ifndef SIFT3D_HIP_H
#define SIFT3D_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIFT3D_DESC_NUMEL 768 /* Include/cSIFT3D.h:27 DESC_NUMEL = 4*4*4*12 */

/* error codes (the reference has none: it prints and carries on, Include/Util/cMemManager.h:35-39) */
enum {
	SIFT3D_OK = 0,
	SIFT3D_ERR_ARG = 1,      /* bad argument */
	SIFT3D_ERR_NO_DEVICE = 2,/* no usable HIP device: the library never falls back to the CPU */
	SIFT3D_ERR_HIP = 3,      /* a HIP runtime call failed (see sift3d_last_error) */
	SIFT3D_ERR_STATE = 4,    /* call out of order (e.g. results requested before run) */
	SIFT3D_ERR_CAPACITY = 5  /* an internal device list overflowed even after regrowing */
};

typedef struct sift3d_ctx *sift3d_handle;

/* Constructor parameters; defaults = Include/cSIFT3D.h:13-20 (factory default args :187-202). */
typedef struct sift3d_params {
	int num_kp_levels;      /* NUM_KP_LEVELS 3 */
	float sigma_default;    /* SIGMA_DEFAULT 1.6 */
	float sigma_n_default;  /* SIGMA_N_DEFAULT 1.15 */
	float peak_thresh;      /* PEAK_THRESH 0.1 */
	float max_eig_thres;    /* EIG_THRES 0.9 */
	float corner_thresh;    /* CORNER_THRESH 0.4 */
} sift3d_params;

/* POD mirror of CPUSIFT::Keypoint without the desc pointer (Include/cSIFT3D.h:54-70): 168 bytes. */
typedef struct sift3d_keypoint {
	float x, y, z;
	float scale;
	int octave, level;
	float rx, ry, rz;
	float win[3];
	float eigvalue[3];
	float eigvector[9];
	float Rotation[9];   /* returned TRANSPOSED after the descriptor stage, like Src/cSIFT3D.cc:1214 */
	float str_tensor[9];
} sift3d_keypoint;
/* layout guard of the record that crosses the boundary (SURVEY 8a-1 lists the offsets of CPUSIFT::Keypoint; this POD is that record
 * without its trailing desc pointer): a compiler / packing change breaks the build, not the results */
#if defined(__cplusplus)
#define SIFT3D_STATIC_ASSERT(c, m) static_assert(c, m)
#else
#define SIFT3D_STATIC_ASSERT(c, m) _Static_assert(c, m)
#endif
SIFT3D_STATIC_ASSERT(sizeof(sift3d_keypoint) == 168, "sift3d_keypoint must be 168 bytes");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_keypoint, scale) == 12 && offsetof(sift3d_keypoint, octave) == 16 && offsetof(sift3d_keypoint, rx) == 24 &&
                     offsetof(sift3d_keypoint, win) == 36 && offsetof(sift3d_keypoint, eigvalue) == 48 && offsetof(sift3d_keypoint, eigvector) == 60 &&
                     offsetof(sift3d_keypoint, Rotation) == 96 && offsetof(sift3d_keypoint, str_tensor) == 132, "sift3d_keypoint field offsets");
SIFT3D_STATIC_ASSERT(sizeof(sift3d_params) == 24, "sift3d_params must be 24 bytes");

void sift3d_default_params(sift3d_params *p);

/* Replaces CSIFT3DFactory::CreateCSIFT3D(float*, nx, ny, nz, ...) + CSIFT3D::CSIFT3D
 * (Src/cSIFT3D.cc:103-110, 146-163): copies the caller's volume (caller keeps ownership), uploads it
 * to `device` and max-abs normalises it there (data_scale, Src/cUtil.cc:536-564).  Also reserves the
 * whole device arena (both pyramids, scratch, keypoint lists) so that sift3d_run allocates nothing.
 * volume_on_device != 0: `volume` is a device pointer on `device` (copied D2D). */
int sift3d_create(sift3d_handle *out, const float *volume, int nx, int ny, int nz,
                  const sift3d_params *params, int device, int volume_on_device);

/* Typed input (no reference counterpart: the reference's callers widen 8 / 16-bit CT and MR voxels to float on the host, e.g.
 * Src/Util/readNii.cpp:17-33).  The library takes the integer voxels as they are stored, moves them at their own width and widens
 * them on the GPU.  Volumes are x fastest like every other volume; `dtype` is one of: */
enum { SIFT3D_DT_F32 = 0, SIFT3D_DT_U8 = 1, SIFT3D_DT_I8 = 2, SIFT3D_DT_U16 = 3, SIFT3D_DT_I16 = 4 };
/* bytes of one voxel: 4 / 1 / 1 / 2 / 2; SIFT3D_ERR_ARG outside the enum.  Host only, no GPU. */
int sift3d_dtype_bytes(int dtype, int *bytes);
/* sift3d_create for a typed volume: the same argument checks (the 2^31 voxel bound included), the same handle, the same everything
 * downstream.  SIFT3D_DT_F32 simply is sift3d_create.  For the integer types a host volume travels through the pinned staging pool
 * as nx*ny*nz*sizeof(T) bytes, beside the allocations like the float volume, into a temporary device buffer of that size; the maximum
 * of |v| is taken in 32-bit integers (-32768 gives 32768) and one kernel widens and divides into the handle's fp32 input.  The
 * temporary is freed before the call returns: the transient device peak is the handle's own memory plus nx*ny*nz*sizeof(T) bytes.
 * volume_on_device != 0: `volume` is a typed device pointer on `device`, any multiple of sizeof(T), read where it lies (no temporary,
 * no copy); as for sift3d_create it must be complete when the call is made.
 * Contract: the handle is BIT FOR BIT the one sift3d_create makes from the same voxels widened to float on the host -- the widening
 * is exact (every 8 / 16-bit integer is an fp32 number), the maximum is the same number (the maximum of the widened |v| is the widened
 * maximum), and the division is the same IEEE division (never a reciprocal multiply; an all-zero volume gives the same 0 / 0).  So
 * sift3d_copy_input, the pyramid, the extrema, the keypoint records and the descriptors are those of the float path.  An integer
 * volume has no NaN or Inf: the handle always runs the fused kernels. */
int sift3d_create_typed(sift3d_handle *out, const void *volume, int dtype, int nx, int ny, int nz,
                        const sift3d_params *params, int device, int volume_on_device);
/* Fills the caller's DEVICE buffer d_dst (nx*ny*nz floats on `device`, any 4-byte alignment: a hipMalloc, a torch tensor) with the
 * unscaled voxels, dst[i] = (float)volume[i]: a plain fp32 device volume that every on_device entry below (sift3d_icgn,
 * sift3d_zncc_search, sift3d_bspline_prefilter, ...) and sift3d_create(volume_on_device = 1) accept, uploaded once and used often.
 * Host inputs of every dtype go through the pinned staging pool (a plain copy of pageable memory moves 0.5-0.8 GB/s on these
 * systems): SIFT3D_DT_F32 straight into d_dst, the integer types at their own width into a grow-only device scratch that stays with
 * the device (nx*ny*nz*sizeof(T) bytes and a quarter), from where one kernel widens them.  volume_on_device != 0: `volume` is a
 * typed device pointer on `device`, read where it lies (SIFT3D_DT_F32: a device copy; volume == d_dst: nothing).  The call runs behind
 * the work queued on the legacy default stream like every on_device entry and returns when d_dst is complete: the pointer is valid for
 * any later call on any stream.  *seconds (may be NULL): device time of the kernel, the upload excluded (SIFT3D_DT_F32 has no kernel: next to 0).
 * SIFT3D_ERR_ARG, before any device call, for a NULL pointer, a dimension < 1, a dtype outside the enum (and 2^40 voxels or more);
 * SIFT3D_ERR_NO_DEVICE behind that check when no GPU is visible -- as sift3d_create_typed. */
int sift3d_volume_to_device(const void *volume, int dtype, int nx, int ny, int nz, int volume_on_device,
                            int device, float *d_dst, double *seconds);

/* Replaces CSIFT3D::~CSIFT3D (Src/cSIFT3D.cc:140-144). */
int sift3d_destroy(sift3d_handle h);

/* Replaces CSIFT3D::KpSiftAlgorithm (Src/cSIFT3D.cc:165-235): whole pipeline, results stay on the
 * device until sift3d_get_keypoints.  Returns after the stream has drained. */
int sift3d_run(sift3d_handle h);

/* KpSiftAlgorithm split in two (no reference counterpart: the reference's call blocks, Src/cSIFT3D.cc:165-235): sift3d_run_async
 * enqueues the whole pipeline on the handle's own streams and returns without waiting; sift3d_wait completes it (results, stage
 * times, the rare list regrow + rerun).  One host thread can keep several handles in flight on one GPU -- BASELINE configs[2] / [4]
 * extract several volumes: the pyramid of one is bound by memory while the descriptors of another are bound by instruction issue.
 * Every accessor of a handle with a run in flight completes it first; sift3d_wait without a run in flight returns SIFT3D_OK. */
int sift3d_run_async(sift3d_handle h);
int sift3d_wait(sift3d_handle h);
/* sift3d_run_async whose pipeline starts when the orientation stage of `after` (a handle with a run in flight on the same GPU) has ended:
 * the memory-bound front of this volume (pyramid, extrema, orientation) runs beside the descriptor stage of the volume before it, which is
 * bound by instruction issue and the LDS (Example.cpp:21-44 extracts two volumes back to back).  after == NULL / nothing in flight: plain
 * sift3d_run_async. */
int sift3d_run_async_after(sift3d_handle h, sift3d_handle after);

/* Replaces calling the public stage methods one by one (Include/cSIFT3D.h:157-165); `upto`:
 * 1 Initialize+Build_Gaussian_Scale_Space(+fused DoG), 2 Build_DOG_Scale_Space, 3 Detect_KeyPoints,
 * 4 Assign_Orientation, 5 Extract_Description.  Used by the parity tests. */
int sift3d_run_stages(sift3d_handle h, int upto);

/* Replaces SIFT_TimerPara m_timer (Include/Util/common.h:22-41; filled Src/cSIFT3D.cc:228-233).
 * Seconds, from HIP events on the handle's stream:
 * t[0] total, t[1] allocation(=0, arena is reserved at create), t[2] GSS(+fused DoG), t[3] DoG(=0 when
 * fused), t[4] detect, t[5] orientation, t[6] description, t[7] release(=0). */
int sift3d_stage_times(sift3d_handle h, double t[8]);

/* Replaces CSIFT3D::GetKeypoints (Src/cSIFT3D.cc:1686-1688).  Order = reference order:
 * (octave, level, z, y, x) scan order (Src/cSIFT3D.cc:373-416, 459-466). */
int sift3d_num_keypoints(sift3d_handle h, int *n);
int sift3d_get_keypoints(sift3d_handle h, sift3d_keypoint *out, float *desc /* n*768, may be NULL */);

/* Device-resident results for a matcher that never leaves the GPU: row-major n*768
 * descriptors and n*3 (rx,ry,rz); valid until the next run / destroy. */
int sift3d_device_results(sift3d_handle h, const float **d_desc, const float **d_xyz, int *n);

/* Checking accessors, replace GET_GSS / GET_DOG / GET_LEVEL (Include/cSIFT3D.h:167-177). */
int sift3d_num_octaves(sift3d_handle h, int *n);
int sift3d_level_info(sift3d_handle h, int is_dog, int idx, int dims3[3], float units3[3], float *scale);
int sift3d_copy_level(sift3d_handle h, int is_dog, int idx, float *out);
int sift3d_copy_input(sift3d_handle h, float *out);
int sift3d_num_extrema(sift3d_handle h, int *n);
int sift3d_get_extrema(sift3d_handle h, sift3d_keypoint *out);
/* per-extremum result code of Assign_Orientation_Imp (1 / -1 / -2 / -3), Src/cSIFT3D.cc:913-1138 */
int sift3d_get_orientation_codes(sift3d_handle h, int *codes);

/* Replaces the free function GaussianSmooth_3D (Include/cSIFT3D.h:212; Src/cSIFT3D.cc:535-622) on a
 * host volume (unit-level parity tests). */
int sift3d_gaussian_smooth(const float *src, int nx, int ny, int nz, float sigma, float *dst, int device);
/* Replaces the free function DownSample_3D (Include/cSIFT3D.h:210; Src/cSIFT3D.cc:506-533): dst(n, m, k) = src(2n, 2m, 2k) for every
 * voxel of the caller-sized dst (2 (nx - 1) < snx etc.), host volumes. */
int sift3d_downsample(const float *src, int snx, int sny, int snz, float *dst, int nx, int ny, int nz, int device);
/* Replaces the free function Sub (Include/cSIFT3D.h:218; Src/cSIFT3D.cc:849-882): dog = (cur - prev) * (-1), n voxels, host volumes. */
int sift3d_dog_sub(const float *prev, const float *cur, size_t n, float *dog, int device);
/* Replaces the free function GaussianSmooth_3D_Imp (Include/cSIFT3D.h:214; Src/cSIFT3D.cc:624-788): ONE pass along `dim` (0 x, 1 y, 2 z)
 * with the caller's taps weight[0 .. width) (width odd, <= 129), interior and mirror-boundary rule as in the pipeline; host volumes. */
int sift3d_conv_axis(const float *src, int nx, int ny, int nz, int dim, const float *weight, int width, float *dst, int device);
/* Replace the free functions Assign_Orientation_Imp / Extract_Descriptor_Imp (Include/cSIFT3D.h:224, 228; Src/cSIFT3D.cc:913-1138,
 * 1152-1381) for ONE keypoint on a caller-provided HOST level (nx x ny x nz, isotropic unit = 2^octave): the pipeline's own kernels run on
 * the box of the level the window reaches.  The keypoint sits on a voxel (integral x, y, z), as every keypoint of the pipeline does;
 * anything else is refused.  orient: in x, y, z, scale; out win, eigvalue, eigvector, Rotation (not transposed), str_tensor and *code =
 * the reference's return value (1 / -1 / -2 / -3).  describe: in x, y, z, scale, Rotation as orientation left it (+ str_tensor: first
 * guess of the fixed-point unit only); out desc768 (normalised) and Rotation TRANSPOSED, like Src/cSIFT3D.cc:1214 leaves it.  The level
 * need not be normalised: any amplitude whose gradients are finite gives the reference's row within the descriptor tolerance, a NaN / Inf
 * gradient in the window its constant row, and a finite gradient whose square overflows (|g| > 1.8e19) the row the reference's float
 * histogram ends as (Inf in the bins that voxel reaches: those bins equal, the others 0) -- describe handles that case in a pass of its
 * own behind the descriptor kernel. */
int sift3d_orient_keypoint(const float *level, int nx, int ny, int nz, float unit, sift3d_keypoint *kp, float sigma, float max_eig_ratio,
                           float corner_thresh, int device, int *code);
int sift3d_describe_keypoint(const float *level, int nx, int ny, int nz, float unit, sift3d_keypoint *kp, float *desc768, int device);

/* Replaces muBruteMatcher::injectMatch / bijectMatch / enhancedMatch (Src/cMatcher.cc:146-228).
 * mode 1 inject, 2 biject, 3 enhanced.  desc: n*768 / m*768, xyz: n*3 / m*3 (rx,ry,rz).
 * on_device != 0: the four input pointers are device pointers on `device`.
 * Outputs (host, any may be NULL): gIdx/sIdx/gDist/sDist sized n = getGlodenIdx / getSilverIdx /
 * getGlodenDistSquare / getSilverDistSquare (Include/cMatcher.h:69-73); pairs6: up to n rows of
 * (ref rx,ry,rz, tar rx,ry,rz) in ascending ref index (toCvec, Src/cMatcher.cc:99-112).
 * Descriptor values: any finite floats are accepted (signed, all-zero rows, exact duplicates, any scaling), the result is the
 * reference's bit for bit.  Its scan is a strict '>' from FLT_MIN (Src/cMatcher.cc:52-77), so a column whose dot product is
 * <= FLT_MIN or NaN is never chosen, and a row with no other column returns index -1 and d = 2 - 2 * FLT_MIN (2.0f) in that place.
 * +-inf / NaN components follow the reference's arithmetic (fp32 product, fp64 sum: inf * 0 and inf - inf are NaN; a +inf score wins,
 * d = -inf, ties keep the lower column).  Outside the contract: magnitudes at which an fp32 product a[k] * b[k] or the fp32 squared
 * norm of a row overflows. */
int sift3d_match(const float *ref_desc, const float *ref_xyz, int n, const float *tar_desc,
                 const float *tar_xyz, int m, double thresHold, int mode, int on_device, int device,
                 int *gIdx, int *sIdx, float *gDist, float *sDist, float *pairs6, int *npairs,
                 double *seconds /* device time of the call, may be NULL */);
/* The same match on the device-resident results of two extractors (sift3d_device_results), wherever they live: handles on one GPU
 * are matched in place; with `tar` on another GPU of the node its descriptors and coordinates are first copied peer to peer (xGMI)
 * into a scratch of `ref` on ref's device.  This is the building block of BASELINE configs[4] for a single-process C++ caller -- N
 * extractors, one per GPU, all ordered pairs (CPUSIFT::CSIFT3D::AllPairsMatch in the C++ shell; 3dsift_amd/dist.py does the same
 * over torch.distributed with an RCCL all-gather, one process per GPU).  Completes runs in flight on both handles first. */
int sift3d_match_handles(sift3d_handle ref, sift3d_handle tar, double thresHold, int mode, int *gIdx, int *sIdx, float *gDist,
                         float *sDist, float *pairs6, int *npairs, double *seconds);
/* times of the calling thread's last sift3d_match: device_seconds = HIP events around the device work on the matcher's stream
 * (what *seconds returned), wall_seconds = host clock around the whole call (scratch reuse, H2D of host inputs, the O(N) host
 * bookkeeping of Src/cMatcher.cc:81-144 and the D2H of the results included) */
int sift3d_match_times(double *device_seconds, double *wall_seconds);
/* muBruteMatcher's constructor (Include/cMatcher.h:30): the matcher's kernels, stream and first scratch exist before the first call */
int sift3d_match_warmup(int device);

int sift3d_device_count(int *n);

/* ------------------------------------------------------------------------------------------------------------
 * Multi-GPU sharding of ONE large volume (no reference counterpart: the reference is single process).
 * Octave 0 is split into z-slabs, one per rank; every level buffer of a slab context holds the owned global planes
 * [z0, z1) plus `halo` planes on each side, which the CALLER fills by exchanging planes with the z-neighbours
 * (3dsift_amd/slab.py does it with torch.distributed P2P over RCCL).  Boundary rules and keypoint coordinates use
 * global z.  Octaves >= 1 run replicated from the all-gathered G[1][0] in a SEEDED context, with the descriptor
 * work split by keypoint slot.  Results equal the single-GPU results bit for bit (pyramid, extrema) / to the
 * descriptor tolerance.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct sift3d_slab_desc {
	int nx, ny, nz;      /* GLOBAL dims of the volume */
	int z0, z1;          /* owned global planes [z0, z1) of this octave; any integers since r06 (the slab of the octave below then owns [ceil(z0/2), ceil(z1/2))) */
	int halo;            /* margin planes per side; >= 38 for default parameters (descriptor window reach) */
	int noct_total;      /* octaves of the ORIGINAL volume: (int)log2f(min dim) - 2 */
	int octave;          /* absolute octave this context holds (0 = the input octave).  octave > 0: nx,ny,nz,z0,z1 are in
	                      * that octave's voxels and G[octave][0] is provided by the caller (owned planes written by
	                      * sift3d_slab_decimate of the octave above, halo planes exchanged); sift3d_slab_level(h, 0) is a no-op */
} sift3d_slab_desc;

/* smallest admissible halo for `params`: the z reach of a descriptor window in octave 0 (38 for the defaults) */
int sift3d_slab_min_halo(const sift3d_params *params, int *halo);
/* r06: *ok = 1 if slab contexts can hold an octave of these GLOBAL dims with these parameters (every level a slab builds takes the z-march kernel:
 * half widths 2 .. 8, planes of 32 or >= 32 + hw voxels per side, at least 2 hw + 2 planes); first_octave != 0: the base blur of the input too */
int sift3d_slab_admits(const sift3d_params *params, int nx, int ny, int nz, int first_octave, int *ok);
/* floats the caller must provide for the level buffers (input, GSS and DoG levels of octave 0) */
int sift3d_slab_arena_floats(const sift3d_slab_desc *d, const sift3d_params *params, size_t *n);
int sift3d_slab_create(sift3d_handle *out, const sift3d_slab_desc *d, const sift3d_params *params, int device,
                       float *d_arena, size_t arena_floats);
/* kind 0 input, 1 GSS level idx, 2 DoG level idx: offset of the buffer inside the arena (floats), planes held and
 * the global z of its plane 0 (= z0 - halo); plane k of the buffer is global plane zoff + k, planes are nx*ny floats */
int sift3d_slab_buffer(sift3d_handle h, int kind, int idx, size_t *offset_floats, int *planes, int *zoff);
/* copy global planes [zg0, zg1) of the RAW volume into the input buffer (host or device source) */
int sift3d_slab_upload(sift3d_handle h, const float *planes, int zg0, int zg1, int on_device);
int sift3d_slab_input_absmax(sift3d_handle h, float *local_max);   /* over the OWNED planes (data_scale pass 1) */
int sift3d_slab_input_scale(sift3d_handle h, float global_max);    /* v /= max on every held plane (pass 2) */
/* GSS level i (and DoG i-1, local max|DoG i-1|) on the owned planes; needs level i-1 (input for i = 0) valid on
 * [z0-hw_i-1, z1+hw_i] -- i.e. after the caller exchanged that many halo planes.  Asynchronous on the handle's stream;
 * sift3d_slab_sync waits. */
int sift3d_slab_level(sift3d_handle h, int i);
int sift3d_slab_level_hw(sift3d_handle h, int i, int *hw);   /* half width of the Gaussian that produces GSS level i */
int sift3d_slab_halo_planes(sift3d_handle h, int gss_level, int *planes); /* planes of GSS level i its consumers need per side */
int sift3d_slab_sync(sift3d_handle h);
/* Stream-ordered driving (no host synchronisation between the levels): every later call of the handle enqueues on the caller's
 * stream (a hipStream_t of the handle's device; NULL = the handle's own stream again); the DoG maxima travel as nd floats in
 * device memory around the caller's MAX all-reduce; the decimation does not wait for completion. */
int sift3d_set_stream(sift3d_handle h, void *hip_stream);
int sift3d_slab_export_dogmax_device(sift3d_handle h, float *d_dst);
int sift3d_slab_import_dogmax_device(sift3d_handle h, const float *d_src);
int sift3d_slab_decimate_async(sift3d_handle h, float *d_dst);
int sift3d_slab_get_dogmax(sift3d_handle h, float *max5);          /* local maxima of the DoG levels (host) */
int sift3d_slab_set_dogmax(sift3d_handle h, const float *max5);    /* global maxima after the all-reduce */
int sift3d_slab_detect(sift3d_handle h);                            /* extrema of the owned planes (DoG halos of 1 plane exchanged) */
int sift3d_slab_describe(sift3d_handle h);                          /* orientation + descriptors; results via sift3d_get_keypoints */
/* r05 -- descriptor windows split along z over the ranks (no reference counterpart: Src/cSIFT3D.cc:484-502 walks whole windows in one
 * process).  Instead of the 24 / 30 / 38-plane halos of G[1..3] that whole windows reach, the ranks exchange keypoint RECORDS
 * (sift3d_slab_record_bytes each) with the z-neighbours within sift3d_slab_desc_reach planes; every rank marches, for its own and for
 * the foreign records, its part of the window planes (sift3d_slab_describe_partial: 768 int32 sums + the part's gradient mass per record);
 * the owner adds the parts' integers -- the sums the single-volume run forms -- and the masses in rank order, and finishes
 * (sift3d_slab_describe_finish).  A record whose fixed-point unit fails is flagged and repeated once by all parts with the exact unit.
 * sift3d_slab_set_desc_partial makes sift3d_slab_halo_planes answer with the orientation window's reach for G[1..levels]. */
int sift3d_slab_set_desc_partial(sift3d_handle h, int on);
/* r06 -- ghost zones: sift3d_slab_level(h, i) then produces level i on [z0 - g_i, z1 + g_i) with g_i shrinking level by level down to what the
 * windows and the extremum test read, from an input (octave 0) or a level 0 (octave > 0) that holds sift3d_slab_min_halo_ghost planes per side --
 * and NO halo of any level has to be exchanged (the exchange between consecutive levels is the one a slab's level chain waits for).  Costs the
 * levels' work on the ghost planes (defaults, 64-plane slabs: + 60 %); every plane holds what its owner computes for it, results unchanged. */
int sift3d_slab_set_ghost(sift3d_handle h, int on);
int sift3d_slab_min_halo_ghost(const sift3d_params *params, int partial_windows, int *halo);
int sift3d_slab_min_halo_partial(const sift3d_params *params, int *halo);  /* planes per side a level buffer needs in that mode */
int sift3d_slab_record_bytes(int *bytes);
int sift3d_slab_desc_reach(sift3d_handle h, int *planes);
int sift3d_slab_orient(sift3d_handle h);                            /* orientation of the owned extrema; then sift3d_num_keypoints */
int sift3d_slab_export_records(sift3d_handle h, void *d_dst);       /* accepted keypoints, processing order, device memory */
/* nlists record lists in one launch: the rank's own keypoints and those of its z-neighbours.  owner_z0/1[i]: the planes list i's owner owns
 * (the owner marches the window planes its level buffers hold, every other rank its owned planes outside that range). */
int sift3d_slab_describe_partial(sift3d_handle h, int nlists, const void *const *d_records, const int *n,
                                 const float *const *d_units /* NULL, or per list NULL / the second round's units */,
                                 int *const *d_hist /* [n[i]][768] each */, float *const *d_mass /* [n[i]] each */, const int *owner_z0,
                                 const int *owner_z1);
int sift3d_slab_describe_finish(sift3d_handle h, const void *d_records, int n, int nparts /* <= 6 */,
                                const int *const *d_hist /* the parts of the n records: the owner's and its neighbours', ascending rank */,
                                const float *const *d_mass, const float *d_units, int final_round, int *d_redo /* [n] out */,
                                float *d_units_next /* [n] out */, int *n_redo);
int sift3d_slab_orient_launch(sift3d_handle h);                     /* sift3d_slab_orient as two calls (several ranks in one process) */
int sift3d_slab_orient_count(sift3d_handle h, int *n_kp);
/* r06 -- the same stages without a host read-back in between (the native driver's critical path): sift3d_slab_keypoints_launch enqueues
 * Detect_KeyPoints + Assign_Orientation of the owned planes and the read-back of their counts; sift3d_slab_keypoints_count waits for it
 * (a list that overflowed is regrown and both stages repeated, blocking).  sift3d_slab_describe_finish_launch is the first round's finish
 * with the count of flagged records read back asynchronously; sift3d_slab_describe_finish_count waits for it (0: results complete). */
int sift3d_slab_keypoints_launch(sift3d_handle h);
int sift3d_slab_keypoints_count(sift3d_handle h, int *n_kp);
int sift3d_slab_describe_finish_launch(sift3d_handle h, const void *d_records, int n, int nparts, const int *const *d_hist,
                                       const float *const *d_mass, int *d_redo /* [n] out */, float *d_units_next /* [n] out */);
int sift3d_slab_describe_finish_count(sift3d_handle h, int *n_redo);
/* whole descriptor windows of the slab's own keypoints from its own level buffers (halo >= sift3d_slab_min_halo), enqueued behind
 * sift3d_slab_keypoints_launch / _count: complete when the handle's stream has drained */
int sift3d_slab_describe_launch(sift3d_handle h);
/* DownSample_3D of the owned planes of G[octave][num_kp_levels] -> d_dst = (nx/2) x (ny/2) x ((z1-z0)/2) floats (device):
 * the owned planes of level 0 of the next octave (a sharded slab context of octave+1, or the all-gather buffer of the tail) */
int sift3d_slab_decimate(sift3d_handle h, float *d_dst);

/* Seeded context: octaves octave_base.. of a volume whose G[octave_base][0] (dims nx,ny,nz) the caller provides */
int sift3d_create_seeded(sift3d_handle *out, int nx, int ny, int nz, int octave_base, int noct_total,
                         const sift3d_params *params, int device);
int sift3d_seed_upload(sift3d_handle h, const float *level0, int on_device);
/* device address of that level 0 (nx*ny*nz floats): a driver that gathers the seed level writes it in place on the stream it gave the
 * handle (sift3d_set_stream) and follows with sift3d_run_async -- no staging copy, no host synchronisation */
int sift3d_seed_buffer(sift3d_handle h, float **d_level0, size_t *floats);
/* only keypoints with slot % world == rank are described by this handle (rows of the others stay zero) */
int sift3d_set_describe_partition(sift3d_handle h, int rank, int world);
/* Partitioned orientation of a replicated context: sift3d_run_partial_orientation runs the pyramid, the extrema scan and
 * Assign_Orientation for the extrema k with k % world == rank only; sift3d_export_orientation_device packs the results as
 * SIFT3D_ORIENT_WORDS int32 words per extremum (zero rows for the extrema of other ranks), so that an integer
 * all-reduce(SUM) over the ranks yields every row exactly; after sift3d_import_orientation_device, sift3d_run_describe
 * runs Extract_Description for this handle's share of the keypoint slots. */
#define SIFT3D_ORIENT_WORDS 34
int sift3d_run_partial_orientation(sift3d_handle h);
int sift3d_export_orientation_device(sift3d_handle h, int *d_dst /* num_extrema * SIFT3D_ORIENT_WORDS */);
int sift3d_import_orientation_device(sift3d_handle h, const int *d_src);
int sift3d_run_describe(sift3d_handle h);
/* D2D copies between the handle's results and caller-owned device buffers (n*768, n*3 floats): lets a communication
 * layer that only addresses its own allocations all-reduce the partitioned descriptor rows and hand them back */
int sift3d_export_device(sift3d_handle h, float *d_desc_dst, float *d_xyz_dst);
int sift3d_import_descriptors_device(sift3d_handle h, const float *d_desc_src);

/* ------------------------------------------------------------------------------------------------------------
 * Native driver of the z-slab sharding (3dsift_amd/csrc/sharded.hip): ONE host volume over the GPUs of a node, with the call
 * shape of the single-GPU path -- create (copy + normalise, Src/cSIFT3D.cc:146-163), run (KpSiftAlgorithm, :165-235), read
 * back (GetKeypoints, :1686-1688; reference order).  devices[ndev]: one rank per listed GPU, halo exchange over RCCL (ncclSend /
 * ncclRecv between z-neighbours over xGMI, one host thread per GPU; librccl is opened at run time).  sim_ranks > 0 (ndev == 1):
 * that many ranks simulated on the one device -- device copies instead of sends -- which is how 1-GPU boxes test the driver.
 * sharded_octaves: octaves split into slabs (0 = every octave of at least 2^22 voxels and 16 planes per rank, at least two); the remaining
 * octaves run ONCE, on the last rank, from a seed level gathered there.
 * Results equal the single-GPU results: pyramid / extrema / orientation bit for bit, descriptors bit for bit as well (integer
 * histograms).  The C++ shell reaches it through CreateCSIFT3D when SIFT3D_DEVICES lists several GPUs.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct sift3d_sharded *sift3d_sharded_handle;
int sift3d_sharded_create(sift3d_sharded_handle *out, const float *volume, int nx, int ny, int nz, const sift3d_params *params,
                          const int *devices, int ndev, int sim_ranks, int sharded_octaves);
/* the same with option bits.  By default (r06) the descriptor windows are split along z over the ranks (records to the z-neighbours, partial
 * integer histograms back: the sift3d_slab_describe_partial / _finish protocol above; level halos of 13 planes), and whole windows on 39-plane
 * halos are what remains for slabs so thin that a window would span more than 6 ranks.  SIFT3D_SHARDED_WHOLE_WINDOWS asks for whole windows
 * always; SIFT3D_SHARDED_PARTIAL_WINDOWS for partial windows or a refusal (no silent change of form).  Same results bit for bit. */
#define SIFT3D_SHARDED_PARTIAL_WINDOWS 1u
#define SIFT3D_SHARDED_WHOLE_WINDOWS 2u
/* r06: the COPY transport instead of RCCL: the same rank threads, streams and plan, but a neighbour's planes / records / histograms are fetched by
 * device copies behind an event the sender recorded (one copy launch per exchange step on one device, hipMemcpyPeerAsync between devices; no
 * communicator, no librccl).  `devices` may then name a device several times -- N rank threads on ONE GPU, which is how the multi-threaded driver
 * is tested on a one-GPU box -- and at most 16 ranks are taken.  Same results bit for bit.  Ignored with sim_ranks > 0. */
#define SIFT3D_SHARDED_COPY_TRANSPORT 4u
/* r06: octave 0 on ghost zones (sift3d_slab_set_ghost): every rank uploads its planes + 33 (defaults) per side of the INPUT and recomputes what it
 * would otherwise receive -- no exchange at all for octave 0 (0.19 of the 0.28 GB a rank receives per side and step at 1024 x 1024 x 512 over 8, and
 * 6 of the 18 exchanges its level chains wait for), for + 0.5 ms of pyramid work per rank.  For nodes whose links, not whose GPUs, bound the step. */
#define SIFT3D_SHARDED_GHOST_OCTAVE0 8u
int sift3d_sharded_create_ex(sift3d_sharded_handle *out, const float *volume, int nx, int ny, int nz, const sift3d_params *params,
                             const int *devices, int ndev, int sim_ranks, int sharded_octaves, unsigned flags);
int sift3d_sharded_run(sift3d_sharded_handle h);
int sift3d_sharded_num_keypoints(sift3d_sharded_handle h, int *n);
int sift3d_sharded_get_keypoints(sift3d_sharded_handle h, sift3d_keypoint *out, float *desc /* n*768, may be NULL */);
/* ranks, sharded octaves, halo planes; seconds[0] = wall time of the last run (KpSiftAlgorithm: the results are complete on the devices),
 * [1] = the same + the read-back of every rank's results and their merge, once sift3d_sharded_get_keypoints has run (r05 counted both in [0]) */
int sift3d_sharded_info(sift3d_sharded_handle h, int *world, int *sharded_octaves, int *halo, double seconds[2]);
/* the plan: descriptor windows split along z in every sharded octave (1) or not (0), and per sharded octave (stage_partial: an octave whose
 * slabs are too thin for the split carries whole windows on wide halos); the rank that also runs the octaves behind the sharded ones, once
 * for the node (-1: the volume has none), and the planes of octave 0 every rank owns (that rank owns fewer) */
int sift3d_sharded_plan(sift3d_sharded_handle h, int *partial_windows, int *tail_rank, int *planes /* [world] or NULL */,
                        int *stage_partial /* [sharded octaves] or NULL */);
/* bytes every rank receives per step: plane halos (from the plan) and -- from the keypoint counts of the last run -- the records and partial
 * histograms of the octaves whose windows are split along z */
int sift3d_sharded_traffic(sift3d_sharded_handle h, double *halo_bytes /* [world] */, double *window_bytes /* [world] */);
const char *sift3d_sharded_error(sift3d_sharded_handle h);
int sift3d_sharded_destroy(sift3d_sharded_handle h);

/* ------------------------------------------------------------------------------------------------------------
 * Detection options of a plain single-volume handle (no reference counterpart: the reference has one extremum rule,
 * IsExtrema_neighbor, Src/cSIFT3D.cc:884-911 -- 8 neighbours: +-x, +-y, +-z in the level and the centre voxel of the levels
 * above and below -- and integer keypoint coordinates).  The defaults are that rule, bit for bit.
 *   neighbours 80: a voxel of DoG level l must be strictly above (maximum) or strictly below (minimum) all 26 neighbours in
 *   level l and all 27 voxels of levels l-1 and l+1 (Lowe's scale-space extremum); threshold, voxel range, keypoint levels and
 *   emit order as in the 8-neighbour rule, so its extrema are a subsequence of the 8-neighbour extrema.
 *   refine 1 (either neighbourhood): a quadratic fit in (x, y, z, s), s = DoG level index, on the 3x3x3x3 block around the
 *   extremum, all in fp64 from the fp32 DoG samples: g_i = 0.5 (D+ - D-), H_ii = (D+ + D-) - 2 D0, H_ij = 0.25 (((D++ - D+-) - D-+) + D--),
 *   delta = -H^-1 g by Gaussian elimination with partial pivoting (axis order x, y, z, s; the first largest |pivot| of the column),
 *   contrast D(x^) = D0 + 0.5 g.delta.  A candidate is REJECTED (it is not an extremum) when a pivot is exactly 0, when
 *   max_offset > 0 and some |delta_i| > max_offset, when contrast_thresh > 0 and |D(x^)| < contrast_thresh * max|level| (fp32
 *   product, like peak_thresh), or when edge_ratio = r > 0 and the spatial 3x3 block of H fails tr det > 0 && tr^3 / det < (2r+1)^3 / r^2
 *   (Allaire et al. 2008).  Keypoints are never moved to another voxel: their records, orientation frames and descriptors are
 *   those of the integer voxel, bit for bit as in a default run; the refined position comes separately (sift3d_get_refined).
 * Only plain handles (sift3d_create) take options: z-slab and seeded contexts refuse them with SIFT3D_ERR_ARG.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct sift3d_detect_options {
	int neighbours;        /* 8 (reference rule, default) or 80 */
	int refine;            /* 0 (default) or 1 */
	float max_offset;      /* default 0.5; <= 0: no offset test */
	float contrast_thresh; /* default 0 (off); relative to max|level| like peak_thresh */
	float edge_ratio;      /* default 0 (off) */
	int reserved[3];       /* must be 0 */
} sift3d_detect_options;
SIFT3D_STATIC_ASSERT(sizeof(sift3d_detect_options) == 32, "sift3d_detect_options must be 32 bytes");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_detect_options, refine) == 4 && offsetof(sift3d_detect_options, max_offset) == 8 &&
                     offsetof(sift3d_detect_options, contrast_thresh) == 12 && offsetof(sift3d_detect_options, edge_ratio) == 16 &&
                     offsetof(sift3d_detect_options, reserved) == 20, "sift3d_detect_options field offsets");

/* refined position of one keypoint (fp64 results rounded to fp32 once): rx = (x + delta_x) * 2^octave -- the factor of
 * sift3d_keypoint.rx --, likewise ry, rz; scale = keypoint scale * 2^(delta_s / num_kp_levels) */
typedef struct sift3d_refined {
	float rx, ry, rz;      /* refined coordinates, same units as sift3d_keypoint.rx */
	float scale;           /* refined scale */
	float offset[4];       /* dx, dy, dz, ds in the keypoint's octave / level units */
	float contrast;        /* D(x^) */
} sift3d_refined;
SIFT3D_STATIC_ASSERT(sizeof(sift3d_refined) == 36, "sift3d_refined must be 36 bytes");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_refined, scale) == 12 && offsetof(sift3d_refined, offset) == 16 && offsetof(sift3d_refined, contrast) == 32,
                     "sift3d_refined field offsets");

/* No reference counterpart (generalises IsExtrema_neighbor, Src/cSIFT3D.cc:884-911): the defaults above; needs no GPU. */
void sift3d_default_detect_options(sift3d_detect_options *o);
/* No reference counterpart (generalises Src/cSIFT3D.cc:884-911): the options of the next run of a plain handle.
 * SIFT3D_ERR_STATE while an asynchronous run is in flight; SIFT3D_ERR_ARG for neighbours not 8 / 80, refine not 0 / 1, a
 * non-finite threshold, a non-zero reserved word, or a z-slab / seeded handle. */
int sift3d_set_detect_options(sift3d_handle h, const sift3d_detect_options *o);
/* No reference counterpart (generalises Src/cSIFT3D.cc:884-911): the options the next run will use. */
int sift3d_get_detect_options(sift3d_handle h, sift3d_detect_options *o);
/* No reference counterpart (generalises Src/cSIFT3D.cc:884-911): num_keypoints records in sift3d_get_keypoints order.
 * SIFT3D_ERR_STATE unless the last completed run had refine on and reached the orientation stage. */
int sift3d_get_refined(sift3d_handle h, sift3d_refined *out);

/* ------------------------------------------------------------------------------------------------------------
 * RANSAC affine fits of matched keypoints (no reference counterpart: the step every caller of enhancedMatch writes next; Rister et al.,
 * "Volumetric Image Registration From Invariant Keypoints").  Input: pairs6, n rows of (ref rx, ry, rz, tar rx, ry, rz) fp32 -- what
 * sift3d_match / sift3d_match_handles return, or any other source of pairs.  A fit is a 3x4 affine t = L r + b.
 *   sift3d_fit_affine: ONE problem whose candidates are all n pairs (problem index p = 0).
 *   sift3d_fit_affine_local: m problems, one per query point q (reference coordinates, p = point index); the candidates of q are the
 *   k nearest pairs by reference position (optionally within `radius`).  Displacement at q: L q + b - q; its gradient: L - I.
 * Numerical contract (fp64 on the fp32 inputs, every expression evaluated in the order written, no FMA contraction, no sqrt before the
 * inlier decision; tests/ransac_ref.py restates it and checks the GPU bit for bit):
 *   Sampler: the 4 draws of hypothesis h (0 <= h < H) of problem p over c >= 4 candidates, uint32 arithmetic mod 2^32, with
 *     fmix32(x) = x ^= x>>16; x *= 0x85ebca6b; x ^= x>>13; x *= 0xc2b2ae35; x ^= x>>16  (murmur3 finaliser):
 *     s = fmix32(seed ^ 0x9E3779B9);  u_j = fmix32(fmix32(s + p) + (4h + j));  i_j = (uint32)(((uint64)u_j * c) >> 32);
 *     while i_j equals an earlier draw of the hypothesis: i_j = (i_j + 1 == c) ? 0 : i_j + 1.
 *     Indices are positions in the problem's candidate list: pair order (global), neighbour order (local).
 *   Minimal solve: samples P0..P3 (ref), T0..T3 (tar); column k-1 of the 3x3 M is P_k - P0, N likewise from T;
 *     cofactor C_rc = +-(M[r1][c1] M[r2][c2] - M[r1][c2] M[r2][c1]) (r1 < r2 the other rows, c1 < c2 the other columns, the sign
 *     (-1)^(r+c) applied by negation); det = (M00 C00 + M01 C01) + M02 C02; DEGENERATE unless |det| >= min_det (NaN: degenerate);
 *     inv_ij = C_ji / det; L_ij = (N_i0 inv_0j + N_i1 inv_1j) + N_i2 inv_2j; b_i = T0_i - ((L_i0 P0x + L_i1 P0y) + L_i2 P0z).
 *   Scoring of a candidate (r, t): e_i = (((L_i0 rx + L_i1 ry) + L_i2 rz) + b_i) - t_i; d2 = (e0 e0 + e1 e1) + e2 e2;
 *     inlier iff d2 <= (double)tau * (double)tau.
 *   Best hypothesis: the non-degenerate one with the most inliers, ties to the smallest h; none: status 2.
 *   Refit (`refine` rounds): on the current inlier set (at least 4, else stop) the means rbar, tbar, Cov = sum (r - rbar)(r - rbar)^T,
 *     S = sum (t - tbar)(r - rbar)^T, L = S Cov^-1 (the cofactor inverse above, L_ij = (S_i0 inv_0j + S_i1 inv_1j) + S_i2 inv_2j),
 *     b = tbar - L rbar (as b_i above); |det Cov| < min_det (or NaN): stop, keep the previous transform, status 3.  Re-scored after
 *     every accepted round.  Sums run in a fixed order of the implementation: two calls give the same bits (checked to tolerance).
 *   Local neighbours of q: fp32 d2_i = (dx dx + dy dy) + dz dz, dx = r_x - q_x; the candidates are the k smallest (d2_i, i) in
 *     lexicographic order among the pairs with d2_i <= radius * radius (fp32; radius <= 0: no limit; a NaN d2_i never qualifies),
 *     listed in that order; 4 <= k <= 64; fewer than 4 candidates: status 1.  A d2_i that overflows to +inf qualifies when there is no
 *     limit (behind every finite one, in index order) and never under a finite radius * radius.
 *   Non-finite values: the expressions above are IEEE operations, so a NaN or an infinity in a pair goes where they carry it (a NaN
 *     in a sampled reference position: degenerate; in a target: a NaN transform that counts no inlier; min_det = 0 accepts det = 0 and
 *     divides by it).  Where A or hyp holds a NaN its position is part of the contract, its sign and payload are unspecified.
 * Results: A = the final transform; hyp = the best hypothesis's minimal-sample transform (bit exact); inliers / rms (sqrt of the mean
 * d2, fp32) over the final inlier set, which the mask holds.  Status 1 / 2 leave A, hyp zero, best_hypothesis -1 and the mask empty:
 * they are results of a successful call, not errors.  SIFT3D_ERR_ARG (checked before any device call): n < 0, m < 0, k outside
 * 4..64, iterations outside 0..65536, refine outside 0..4, tau or min_det negative or not finite, radius not finite, a non-zero
 * reserved word, a NULL pointer that is needed (options may be NULL: defaults).  on_device != 0: pairs6 / points3 are device pointers
 * on `device`; outputs are host memory, filled by one copy at the end.  *seconds (may be NULL): device time of the call (HIP events).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct sift3d_ransac_options {
	int iterations;        /* hypotheses per problem; 0 = default: 4096 global, 256 local; max 65536 */
	float inlier_thresh;   /* tau, in rx units (full-resolution voxels); default 3.0 */
	unsigned seed;         /* default 1 */
	int refine;            /* refit rounds 0..4, default 1 */
	float min_det;         /* default 1.0 */
	int reserved[3];       /* must be 0 */
} sift3d_ransac_options;
SIFT3D_STATIC_ASSERT(sizeof(sift3d_ransac_options) == 32, "sift3d_ransac_options must be 32 bytes");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_ransac_options, inlier_thresh) == 4 && offsetof(sift3d_ransac_options, seed) == 8 &&
                     offsetof(sift3d_ransac_options, refine) == 12 && offsetof(sift3d_ransac_options, min_det) == 16 &&
                     offsetof(sift3d_ransac_options, reserved) == 20, "sift3d_ransac_options field offsets");

typedef struct sift3d_affine_fit {
	double A[12];          /* final transform, row-major 3x4: [L | b] */
	double hyp[12];        /* the best hypothesis's minimal-sample transform (bit exact against the contract) */
	int status;            /* 0 ok, 1 fewer than 4 candidates (rigid fits: 3), 2 every hypothesis degenerate, 3 refit singular */
	int candidates;        /* pairs the problem drew from (n, or the neighbours found) */
	int best_hypothesis;   /* h of the best hypothesis, -1 with status 1 / 2 */
	int best_count;        /* its inliers */
	int inliers;           /* inliers of A */
	float rms;             /* sqrt(mean d2) over the final inliers */
	int reserved[2];
} sift3d_affine_fit;
SIFT3D_STATIC_ASSERT(sizeof(sift3d_affine_fit) == 224, "sift3d_affine_fit must be 224 bytes");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_affine_fit, hyp) == 96 && offsetof(sift3d_affine_fit, status) == 192 &&
                     offsetof(sift3d_affine_fit, candidates) == 196 && offsetof(sift3d_affine_fit, best_hypothesis) == 200 &&
                     offsetof(sift3d_affine_fit, best_count) == 204 && offsetof(sift3d_affine_fit, inliers) == 208 &&
                     offsetof(sift3d_affine_fit, rms) == 212 && offsetof(sift3d_affine_fit, reserved) == 216, "sift3d_affine_fit field offsets");

/* the defaults above; needs no GPU */
void sift3d_default_ransac_options(sift3d_ransac_options *o);
/* the global fit; inlier_mask: n bytes (1 inlier of A, 0 not), may be NULL */
int sift3d_fit_affine(const float *pairs6, int n, const sift3d_ransac_options *o, int on_device, int device, sift3d_affine_fit *out,
                      unsigned char *inlier_mask, double *seconds);
/* m local fits; out: m records; neighbours: m*k pair indices in candidate order, -1 padded, may be NULL */
int sift3d_fit_affine_local(const float *pairs6, int n, const float *points3, int m, int k, float radius, const sift3d_ransac_options *o,
                            int on_device, int device, sift3d_affine_fit *out, int *neighbours, double *seconds);

/* ------------------------------------------------------------------------------------------------------------
 * RANSAC rigid and similarity fits of matched keypoints (no reference counterpart; Rister et al. fit rigid transforms before affine
 * ones; Horn, "Closed-form solution of absolute orientation using unit quaternions").  model 0: rigid, t = R r + b with R a proper
 * rotation; model 1: similarity, t = s R r + b, s > 0.  Input, options, record, statuses, neighbour lists, on_device and *seconds are
 * those of the affine fits above; A and hyp hold [s R | b], so sift3d_icgn_init_from_fits and everything after it take the record
 * unchanged.  A fit needs 3 candidates: status 1 means fewer than 3, and 3 <= k <= 64.  A rotation is fixed by 3 pairs that are not
 * collinear, so coplanar pairs -- where every affine hypothesis is degenerate -- are fitted.
 * Numerical contract (fp64 on the fp32 inputs, every expression evaluated in the order written, no FMA contraction, sqrt and / are the
 * correctly rounded IEEE operations; tests/rigid_ref.py restates it and checks the GPU bit for bit on hyp):
 *   u.v = (u0 v0 + u1 v1) + u2 v2;  u x v = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0).
 *   Sampler: draws 0..2 of the affine sampler (u_j = fmix32(fmix32(s + p) + (4h + j)), j < 3, the duplicate rule among these three);
 *     its draw 3 is not made, so c = 3 candidates are drawn in some order of the three.
 *   Minimal solve (triad): samples P0..P2 (ref), T0..T2 (tar); a = P1 - P0, b = P2 - P0, c = a x b; x = a / sqrt(a.a),
 *     z = c / sqrt(c.c), y = z x x; a', b', c', x', y', z' alike from T.  DEGENERATE unless c.c >= min_det * min_det and c'.c' > 0
 *     (NaN: degenerate): min_det bounds twice the area of the sample's triangle.  R_ij = (x'_i x_j + y'_i y_j) + z'_i z_j.
 *     Rigid: L = R.  Similarity: s = sqrt(((a'.a' + b'.b') + (b' - a').(b' - a')) / ((a.a + b.b) + (b - a).(b - a))), L_ij = s R_ij.
 *     b_i = T0_i - ((L_i0 P0x + L_i1 P0y) + L_i2 P0z).
 *   Scoring, threshold and best hypothesis: those of the affine fits.
 *   Refit (`refine` rounds, Horn's quaternion method): on the current inlier set (at least 3, else stop) the means rbar, tbar; with
 *     d = r - rbar, e = t - tbar the sums Cov = sum d d^T, S_ab = sum d_a e_b, E = sum e.e.
 *     e2 = ((C00 C11 - C01 C01) + (C00 C22 - C02 C02)) + (C11 C22 - C12 C12); unless e2 >= min_det * min_det (NaN included: collinear
 *     inliers) stop, keep the previous transform, status 3 (for 3 points e2 = c.c / 3: the units of the sample's rule).
 *     The symmetric 4x4 N: N00 = (Sxx + Syy) + Szz, N11 = (Sxx - Syy) - Szz, N22 = (-Sxx + Syy) - Szz, N33 = (-Sxx - Syy) + Szz,
 *     N01 = Syz - Szy, N02 = Szx - Sxz, N03 = Sxy - Syx, N12 = Sxy + Syx, N13 = Szx + Sxz, N23 = Syz + Szy.
 *     Eigenvectors by cyclic Jacobi, V = I at the start, 8 sweeps over the planes (p, q) = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); a plane
 *     with N_pq == 0 is skipped, else theta = (N_qq - N_pp) / (2 N_pq), t = (theta >= 0 ? 1 : -1) / (|theta| + sqrt(theta theta + 1))
 *     (theta theta may overflow: t = +-0), c = 1 / sqrt(t t + 1), s = t c; N_pp -= t N_pq, N_qq += t N_pq, N_pq = 0; for the other rows r:
 *     (N_rp, N_rq) <- (c N_rp - s N_rq, s N_rp + c N_rq); for every row r of V: (V_rp, V_rq) <- (c V_rp - s V_rq, s V_rp + c V_rq).
 *     q = (w, x, y, z) = the column of V under the largest diagonal entry of N (ties: the lowest index), divided by
 *     sqrt(((q0 q0 + q1 q1) + q2 q2) + q3 q3).  R00 = ((ww + xx) - yy) - zz, R11 = ((ww - xx) + yy) - zz, R22 = ((ww - xx) - yy) + zz,
 *     R01 = 2 (xy - wz), R10 = 2 (xy + wz), R02 = 2 (xz + wy), R20 = 2 (xz - wy), R12 = 2 (yz - wx), R21 = 2 (yz + wx): even in q, so its
 *     sign does not matter.  Rigid: L = R.  Similarity: s = sqrt(E / ((C00 + C11) + C22)), L_ij = s R_ij.  b = tbar - L rbar (as b_i
 *     above).  Re-scored after every accepted round.  Sums run in a fixed order of the implementation: two calls give the same bits
 *     (A is checked to tolerance).
 *   Non-finite values go where these IEEE operations carry them: a NaN in a sampled position makes the sample degenerate, an infinity
 *     in a sampled target gives a NaN transform that counts no inlier; min_det = 0 accepts c.c = 0 and divides by it.
 * SIFT3D_ERR_ARG (checked before any device call): what the affine fits refuse, with k outside 3..64, and model outside 0..1.
 * ------------------------------------------------------------------------------------------------------------ */
/* the global fit; inlier_mask: n bytes (1 inlier of A, 0 not), may be NULL */
int sift3d_fit_rigid(const float *pairs6, int n, int model, const sift3d_ransac_options *o, int on_device, int device,
                     sift3d_affine_fit *out, unsigned char *inlier_mask, double *seconds);
/* m local fits; out: m records; neighbours: m*k pair indices in candidate order, -1 padded, may be NULL */
int sift3d_fit_rigid_local(const float *pairs6, int n, const float *points3, int m, int k, float radius, int model,
                           const sift3d_ransac_options *o, int on_device, int device, sift3d_affine_fit *out,
                           int *neighbours, double *seconds);
/* One fit per body (what "discrete DVC" of a granular specimen reports: the rigid motion of every grain, fitted from the grain's own
 * matched keypoints).  pair_label[i] says which body pair i belongs to -- sift3d_labels_at_positions on the reference positions gives
 * it from the labels of sift3d_mask_label.
 *   Body L (1 <= L <= count) is one problem of the contract above with problem index p = L.  Its candidates are the pairs i with
 *   pair_label[i] == L, in ascending i; c is their number.  A pair whose label is <= 0 or > count belongs to no body.
 *   Everything else is sift3d_fit_rigid's contract word for word: draw<3> over c (u_j = fmix32(fmix32(s + L) + (4h + j))), the triad,
 *   the scoring and the best hypothesis (the most inliers, ties to the smallest h), the Horn refit rounds, status 1 (c < 3), 2 and 3,
 *   and how NaN and Inf travel.  o->iterations = 0 means 256, the local fits' default.
 *   out[L-1] is body L's record, with candidates = c.  inlier_mask[i] (may be NULL) is 1 iff pair i is an inlier of its own body's
 *   final A; it is 0 for a pair of no body and for a body with status 1 or 2.
 *   Two calls return the same bytes.  Body L's record and mask bytes depend only on body L's pairs and their relative order: not on the
 *   other bodies' pairs (non-finite ones included), nor on where in the list its own pairs stand.  A body's refit sums run in the
 *   order of the global fit's on the same list.
 * SIFT3D_ERR_ARG (checked before any device call): sift3d_fit_rigid's rules, count < 0, a NULL pair_label with n > 0, a NULL out with
 * count > 0 (out may be NULL when count is 0).  n = 0 or count = 0 succeed (every record has status 1, every mask byte is 0).
 * on_device != 0: pairs6 and pair_label are device pointers on `device`; out and inlier_mask are host memory.  The labels are brought
 * to the host and the pairs' indices are grouped by body there (a stable counting sort), so the call holds 8 bytes per pair and 4 per
 * body of pinned host memory beside the records; *seconds is the device time of the kernel. */
int sift3d_fit_rigid_bodies(const float *pairs6, int n, const int *pair_label /* n */, int count, int model,
                            const sift3d_ransac_options *o, int on_device, int device,
                            sift3d_affine_fit *out /* count records, host */, unsigned char *inlier_mask /* n, host, may be NULL */,
                            double *seconds);
/* host only, no GPU: per fit the unit quaternion (w, x, y, z; w >= 0) of the rotation, the scale s = cbrt(det L) and the rotation
 * angle 2 atan2(sqrt(xx + yy + zz), w) in degrees of the linear part L of A: R = L / s, q from R by Shepperd's branch on the largest
 * of (trace, R00, R11, R22).  Meant for rigid and similarity fits; a fit with status != 0 gives NaN.  quat4: 4 m doubles, scale and
 * angle_deg: m each.  SIFT3D_ERR_ARG: m < 0, or a NULL pointer with m > 0. */
int sift3d_fit_rotation(const sift3d_affine_fit *fits, int m, double *quat4, double *scale, double *angle_deg);

/* ------------------------------------------------------------------------------------------------------------
 * Guided matching (no reference counterpart for the gate: the step registration pipelines take after a first fit -- match again
 * where the fit says the partner must be, then refit).  sift3d_match's ratio test compares a row's best target with the second best
 * anywhere in the volume; where texture repeats, the true partner and a look-alike far away score alike and the pair is rejected.
 * sift3d_match_guided is sift3d_match with three additions: pred_xyz (n x 3 fp32, the place in the target where reference keypoint i
 * is expected), radius, and the optional per-row output `candidates`.
 *   The gate: gate(i) = { j : fabsf(tar_xyz[j][c] - pred_xyz[i][c]) <= radius for c = 0, 1, 2 }, evaluated in fp32 exactly as written
 *     (one rounded subtraction per component).  A position with a non-finite coordinate, predicted or target, is in no gate and has
 *     an empty one (the comparison is false); so is a position with a coordinate beyond +-2^24, the bound of the spatial index the
 *     gates are found with.  0 < radius <= 2^20, finite.
 *   Forward pass: row i gets what muBruteMatcher::calMatches (Src/cMatcher.cc:40-79) returns when the target set is gate(i) in
 *     ascending j: score s += (double)(a[k] * b[k]) with k ascending, strict '>' from FLT_MIN, ties keep the lower column,
 *     d = 2 - 2 s stored as float, an empty place holds index -1 and d = 2 - 2 * FLT_MIN (2.0f).  The value contract written at
 *     sift3d_match above holds word for word: a column whose score is NaN or <= FLT_MIN is never chosen, +-inf / NaN components
 *     follow the reference's arithmetic.
 *   Modes and bookkeeping: the ratio filter and the modes 1 / 2 / 3 are the reference's (Src/cMatcher.cc:81-144), unchanged.  In modes
 *     2 and 3 the reverse pass of a masked target j scans { i : j in gate(i) } in ascending i -- the same relation transposed, so the
 *     bijection test stays symmetric.  pairs6, npairs, gIdx, sIdx, gDist, sDist and seconds are as in sift3d_match; candidates[i]
 *     (n ints, may be NULL) = |gate(i)|.
 *   A row with ONE candidate has sIdx = -1 and sDist = 2.0f, so it passes the ratio filter when gDist / 2 < thresHold * thresHold:
 *     alone in its gate, a target is accepted on its distance alone.
 *   Consequences: with a gate that holds every target the call returns sift3d_match's bytes in every mode; in mode 1 a pair that
 *     sift3d_match accepts and whose target lies in the row's gate is accepted by the guided call as well whenever sDist > 0 (the second
 *     best inside the gate is no closer than the second best anywhere).
 * on_device != 0: the five input tables are device pointers on `device`; outputs are host memory.  Two calls return the same bytes.
 * SIFT3D_ERR_ARG (checked before any device call): n < 0, m < 0, mode outside 1..3, radius not in (0, 2^20] (NaN included), a NULL
 * table that has rows.  n = 0 or m = 0 succeeds with empty gates.  Above a radius where the gates hold a large share of the targets
 * the brute-force pass of sift3d_match is the faster one (DESIGN 4.5a has the measured crossover).
 * ------------------------------------------------------------------------------------------------------------ */
int sift3d_match_guided(const float *ref_desc, const float *ref_xyz, int n, const float *tar_desc, const float *tar_xyz, int m,
                        const float *pred_xyz, float radius, double thresHold, int mode, int on_device, int device, int *gIdx,
                        int *sIdx, float *gDist, float *sDist, int *candidates, float *pairs6, int *npairs,
                        double *seconds /* device time of the call, may be NULL */);
/* host only, no GPU: where the fits send the reference positions xyz3 (n x 3 fp32: rx, ry, rz).  pred = A (r, 1) in fp64,
 * ((A_i0 rx + A_i1 ry) + A_i2 rz) + A_i3, rounded to float.  nfits is 1 (one global fit for all rows) or n (row i takes fits[i]: the
 * local fits queried at the keypoints' own coordinates).  A fit with a non-zero status gives a NaN row, whose gate is empty.  Takes
 * affine, rigid and similarity records alike.  SIFT3D_ERR_ARG: n < 0, nfits neither 1 nor n, or a NULL pointer with n > 0. */
int sift3d_predict_positions(const sift3d_affine_fit *fits, int nfits, const float *xyz3, int n, float *pred3);

/* ------------------------------------------------------------------------------------------------------------
 * IC-GN displacement refinement for digital volume correlation (no reference counterpart: what the DVC users of the reference run on
 * the initial guess of sift3d_fit_affine_local; Pan et al., inverse-compositional Gauss-Newton with a first-order shape function).
 * Numerical contract (a tolerance contract, not bit for bit; tests/icgn_ref.py restates it in NumPy fp64):
 *   Volumes: fp32, [z][y][x], x fastest (the layout of sift3d_create, the frame of a keypoint's rx, ry, rz).  The reference R and the
 *     target T may differ in size.  A point of interest (POI) is an integer voxel q = (x, y, z) of R.
 *   Shape function: p = (u, ux, uy, uz, v, vx, vy, vz, w, wx, wy, wz); the subset offset d maps to q + F d + (u, v, w) in T with
 *     F = [[1+ux, uy, uz], [vx, 1+vy, vz], [wx, wy, 1+wz]]; M(p) = [[F, (u,v,w)^T], [0, 0, 0, 1]].  From an affine fit A = [L | b] at q:
 *     (u, v, w) = L q + b - q, F = L (sift3d_icgn_init_from_fits).
 *   Subset: d in [-r, r]^3, N = (2r+1)^3 voxels.  Gradient of R: fp32 central differences at integer voxels, Rx = 0.5f * (R[x+1] - R[x-1])
 *     (y, z alike), so the subset plus a 1-voxel margin must lie inside R.  Steepest-descent row of a voxel:
 *     SD = (Rx, Rx dx, Rx dy, Rx dz, Ry, Ry dx, Ry dy, Ry dz, Rz, Rz dx, Rz dy, Rz dz);  H = sum SD^T SD;  Rm = mean of R over the
 *     subset;  dR = sqrt(sum (R - Rm)^2).
 *   Interpolation of T: 0 (default) tricubic Keys convolution, a = -0.5 (Catmull-Rom), 64 taps, weights for the fraction t:
 *     w-1 = (-t^3 + 2t^2 - t)/2, w0 = (3t^3 - 5t^2 + 2)/2, w1 = (-3t^3 + 4t^2 + t)/2, w2 = (t^3 - t^2)/2;  1 trilinear.  A position is in
 *     the domain when every tap lies in T: floor(x) - 1 >= 0 and floor(x) + 2 <= n - 1 per axis (cubic), floor(x) >= 0 and
 *     floor(x) + 1 <= n - 1 (linear).  The warped subset is the affine image of a box: its 8 corners decide.
 *   Iteration: at the current p, Tm, dT = sqrt(sum (T(W) - Tm)^2) and the ZNSSD step
 *     dp = -H^-1 sum SD^T [(R - Rm) - (dR/dT)(T(W) - Tm)];  then M(p) <- M(p) . M(dp)^-1, fp64.  Stop when
 *     ||dp||_r = sqrt(du^2 + dv^2 + dw^2 + r^2 * (sum of the 9 squared gradient terms of dp)) < tolerance.  `iterations` counts the
 *     updates applied; tolerance 0 runs exactly max_iterations updates (status 1).
 *   zncc = sum (R - Rm)(T - Tm) / (dR dT), evaluated at the returned p.
 *   Status per POI (results of a successful call, not errors), checked in this order:
 *     5 init not finite;  2 subset + margin outside R;  4 flat subset (dR = 0, or H not positive definite: a Cholesky pivot <= 0 or NaN)
 *       -- these three return the init as given, iterations 0, zncc 0;
 *     3 warped subset outside T's domain, at the start (init, iterations 0, zncc 0) or after a step (the last in-domain p);
 *     6 a non-finite dp or a singular M(dp) (the last p);  4 dT = 0 during the iteration, to rounding: dT^2 <= 1e-10 sum (T - Rm)^2
 *       (the last p);
 *     1 max_iterations reached without convergence (the last p);  0 converged (the final p).
 *   Precision: per-voxel interpolation in fp32 (the fraction, the weights, every product and sum; a position whose fp32 form rounds
 *   onto the next integer at T's edge is read with fraction 1 from the last admissible base tap: the domain is the fp64 test's); the
 *   sums over the subset are formed with T shifted by Tc, the voxel of T under the subset's centre (ZNSSD does not change when T is
 *   shifted), and the taps are shifted before they are weighted: a constant T has dT = 0 exactly, and scaling T by a power of two
 *   returns the same bits.  The sums are reduced in a fixed order with no float atomics: two calls return the same bits.
 * SIFT3D_ERR_ARG (checked before any device call): m < 0, a dimension < 1, an option outside its range or a non-zero reserved word,
 * NULL ref / tar / out, NULL points3 with m > 0; m = 0 succeeds.  o may be NULL (defaults).  on_device != 0: ref, tar, points3 and
 * init12 are device pointers on `device`; out is host memory, filled by one copy at the end.  *seconds (may be NULL): device time
 * of the call (HIP events; the uploads of host inputs excluded).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct sift3d_icgn_options {
	int subset_radius;     /* r, 2..32, default 16 */
	int max_iterations;    /* 1..100, default 20 */
	float tolerance;       /* >= 0, finite, default 1e-3; 0: run max_iterations updates */
	int interpolation;     /* 0 tricubic Keys (default), 1 trilinear */
	int reserved[4];       /* must be 0 */
} sift3d_icgn_options;
SIFT3D_STATIC_ASSERT(sizeof(sift3d_icgn_options) == 32, "sift3d_icgn_options must be 32 bytes");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_icgn_options, max_iterations) == 4 && offsetof(sift3d_icgn_options, tolerance) == 8 &&
                     offsetof(sift3d_icgn_options, interpolation) == 12 && offsetof(sift3d_icgn_options, reserved) == 16,
                     "sift3d_icgn_options field offsets");

typedef struct sift3d_icgn_result {
	double p[12];          /* u ux uy uz v vx vy vz w wx wy wz */
	double zncc;
	double last_step;      /* ||dp||_r of the last computed step (0: none) */
	int iterations;        /* updates applied */
	int status;            /* the table above */
	int reserved[2];
} sift3d_icgn_result;
SIFT3D_STATIC_ASSERT(sizeof(sift3d_icgn_result) == 128, "sift3d_icgn_result must be 128 bytes");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_icgn_result, zncc) == 96 && offsetof(sift3d_icgn_result, last_step) == 104 &&
                     offsetof(sift3d_icgn_result, iterations) == 112 && offsetof(sift3d_icgn_result, status) == 116 &&
                     offsetof(sift3d_icgn_result, reserved) == 120, "sift3d_icgn_result field offsets");

/* the defaults above; needs no GPU */
void sift3d_default_icgn_options(sift3d_icgn_options *o);
/* host only: m rows of 12 initial parameters from m affine fits at the integer points (x, y, z); a fit with status != 0 gives a NaN
 * row (POI status 5).  SIFT3D_ERR_ARG: m < 0, or a NULL pointer with m > 0. */
int sift3d_icgn_init_from_fits(const sift3d_affine_fit *fits, const int *points3, int m, double *init12);
/* m POIs (x, y, z int triples) refined between ref (rnx x rny x rnz) and tar (tnx x tny x tnz); init12: m*12 or NULL (zero) */
/* host only, no GPU: row i is what sift3d_icgn_init_from_fits writes for (fits[poi_label[i] - 1], point i); a label outside 1..count
 * gives a NaN row, as a failed fit does.  fits: the count records of sift3d_fit_rigid_bodies.  SIFT3D_ERR_ARG: m < 0, count < 0, a NULL
 * fits with count > 0, a NULL poi_label, points3 or init12 with m > 0. */
int sift3d_icgn_init_from_body_fits(const sift3d_affine_fit *fits, int count, const int *poi_label, const int *points3, int m, double *init12);
int sift3d_icgn(const float *ref, int rnx, int rny, int rnz, const float *tar, int tnx, int tny, int tnz, const int *points3, int m,
                const double *init12, const sift3d_icgn_options *o, int on_device, int device, sift3d_icgn_result *out, double *seconds);

/* ------------------------------------------------------------------------------------------------------------
 * Cubic B-spline interpolation of the target (no reference counterpart: the interpolation DVC codes use, because the bias of the
 * Keys kernel limits IC-GN's accuracy).  A prefilter turns a volume into its B-spline coefficients; sift3d_icgn_bspline is
 * sift3d_icgn with the B-spline weights applied to them.
 * Numerical contract of the prefilter (a tolerance contract; tests/bspline_ref.py restates it in NumPy): dst receives the cubic
 * B-spline coefficients of src (fp32, [z][y][x]) with a mirror (whole-sample symmetric) boundary -- scipy.ndimage.spline_filter(
 * order=3, mode="mirror") to fp32 accuracy -- as a truncated, differenced FIR, not the recursion:
 *   z1 = sqrt(3) - 2, K = 16;  h_k = z1^k / (1 + 2 sum_{j=1..K} z1^j) for k = 1..K, formed in fp64 and rounded to fp32 (the 2K + 1
 *     weights sum to 1; the central one is implied).
 *   Per axis, x then y then z, every intermediate volume stored as fp32:
 *     c[i] = s[i] + sum_{k=K..1} h_k * ((s[m(i - k)] - s[i]) + (s[m(i + k)] - s[i])),
 *     m the mirror index map of period 2n - 2 (m(-j) = j, m(n - 1 + j) = n - 1 - j, folded repeatedly when n <= K; m = 0 when n = 1).
 *   Products and sums are fp32, not fused, the sum over k accumulated from k = K down to 1 and added to s[i] last.  No float
 *     atomics and a fixed order: two calls return the same bytes.
 *   Every operation being fixed, dst has the bytes of the restatement's float32 form (bspline_ref.prefilter(T, f32=True)) -- tested
 *     at every seam of the kernel's 64 x 64 tiles along each axis, on axes of length 1 to 17 and with all seams at once, on inputs
 *     whose intermediates are zero or normal (tests/test_gpu_bspline_edges.py).  The tolerance against the fp64 form of the filter
 *     stays as the accuracy statement.
 *   Consequences: a constant volume returns itself bit for bit; an axis of length 1 is the identity (on finite values); a single
 *     non-finite voxel in the interior makes exactly the (2K+1)^3 cube around it non-finite and nothing outside that cube changes;
 *     the truncated tail (|z1|^17 = 1.9e-10) is below fp32 resolution: the fp64 form of this formula differs from the exact filter
 *     by at most 2.8e-8 max|src| (measured on noise).
 * SIFT3D_ERR_ARG (checked before any device call): NULL src / dst, dst == src, a dimension < 1, or a volume too large for a pass:
 * ny * nz >= 2^31, or more than 2^24 - 1 tiles of 64 x 64 voxels in a pass (about 6.8e10 voxels).  SIFT3D_ERR_NO_DEVICE after that
 * check when no GPU is visible: there is no CPU fallback.  on_device != 0: src and dst are device pointers on `device`, ordered
 * behind the legacy default stream; otherwise both are host memory.  Only dst == src is checked: volumes that overlap in part
 * give undefined results.  The call keeps one more volume of src's size on the device (three for host volumes).  *seconds (may be NULL):
 * device time of the call (HIP events; the upload of a host input excluded).
 *
 * sift3d_icgn_bspline: the contract of sift3d_icgn -- the gradient of R, H, the update, the status table, the cubic domain rule
 * (taps floor - 1 .. floor + 2) -- with one difference: T(x) is the tensor product of the cubic B-spline weights
 *     w-1 = (1 - t)^3 / 6, w0 = (3t^3 - 6t^2 + 4) / 6, w1 = (-3t^3 + 3t^2 + 3t + 1) / 6, w2 = t^3 / 6
 * applied to the coefficients of T.  tar_is_coefficients 0: tar is the volume and the call prefilters it into its own scratch (it
 * then holds up to two more volumes of T's size on the device, and *seconds includes the prefilter); 1: tar already holds
 * sift3d_bspline_prefilter's output (prefilter once, refine often).  The centring carries over: Tc is the coefficient at the base
 * tap of the subset's centre and the taps are shifted before they are weighted; a constant T has constant coefficients exactly, so
 * a constant T still has dT = 0 exactly, and scaling T by a power of two still returns the same bits.  A non-finite voxel of T
 * reaches the POIs whose warped subset comes within K + 2 voxels of it (Chebyshev) and no other.
 * SIFT3D_ERR_ARG: as sift3d_icgn, and o->interpolation != 0 (the option has no meaning here; 1 is refused) or tar_is_coefficients
 * outside 0..1.  sift3d_icgn itself is unchanged: it refuses interpolation = 2.
 * ------------------------------------------------------------------------------------------------------------ */
int sift3d_bspline_prefilter(const float *src, int nx, int ny, int nz, float *dst, int on_device, int device, double *seconds);
int sift3d_icgn_bspline(const float *ref, int rnx, int rny, int rnz, const float *tar, int tnx, int tny, int tnz, const int *points3, int m,
                        const double *init12, const sift3d_icgn_options *o, int tar_is_coefficients, int on_device, int device,
                        sift3d_icgn_result *out, double *seconds);

/* ------------------------------------------------------------------------------------------------------------
 * Second-order IC-GN (no reference counterpart: the 30-parameter shape function of DVC codes, for subsets across which the
 * displacement gradient varies -- bending, indentation, the neighbourhood of cracks and inclusions -- where the first-order fit is
 * biased by about kappa r (r + 1) / 6 for a second derivative kappa).  Intended use: sift3d_icgn, sift3d_icgn2_init_from_icgn,
 * sift3d_icgn2.  Numerical contract (a tolerance contract; tests/icgn2_ref.py restates it in NumPy fp64).  Everything not named here
 * is the contract of sift3d_icgn / sift3d_icgn_bspline word for word: the volumes and POIs, the fp32 central-difference gradient of
 * R, Rm and dR, the three interpolations and their tap domains, the centring by Tc with the shift applied before the weights, the
 * fp32 per-voxel arithmetic and the clamp at T's edge, zncc, no float atomics and two calls returning the same bytes.
 *   Parameters: p[30], ten per component in the order u, v, w: (c, cx, cy, cz, cxx, cyy, czz, cxy, cxz, cyz) -- the displacement and
 *     its first and second derivatives at q.  The subset offset d maps, per axis a, to
 *       q_a + d_a + c + cx dx + cy dy + cz dz + 1/2 cxx dx^2 + 1/2 cyy dy^2 + 1/2 czz dz^2 + cxy dx dy + cxz dx dz + cyz dy dz.
 *   Steepest-descent row: SD = (Rx xi', Ry xi', Rz xi') with xi'(d) = (1, dx, dy, dz, 1/2 dx^2, 1/2 dy^2, 1/2 dz^2, dx dy, dx dz, dy dz);
 *     H = sum SD^T SD is 30 x 30, formed in fp64; status 4 by the same column Cholesky, with 30 pivots (a pivot <= 0 or NaN).
 *   Step: dp = -H^-1 sum SD^T [(R - Rm) - (dR/dT)(T(W) - Tm)], fp64.
 *   Update: with xi(d) = (1, dx, dy, dz, dx^2, dy^2, dz^2, dx dy, dx dz, dy dz), M(p) is the 10 x 10 matrix with
 *     xi(W(d) - q) ~ M(p) xi(d): row 0 is e_0; rows 1..3 are the coefficient vectors of the three position polynomials (e_{1+a} plus
 *     the parameters, the squares carrying their 1/2); rows 4..9 are the products of rows (x,x), (y,y), (z,z), (x,y), (x,z), (y,z) as
 *     polynomials in d with every term of degree 3 or 4 dropped.  M(p) <- M(p) . M(dp)^-1 in fp64; the new p is read from rows 1..3.
 *     Status 6: a non-finite dp, or a singular M(dp): an LU pivot (partial pivoting by rows, the first entry of largest magnitude)
 *     that is 0 or not finite.
 *   Stopping norm: ||dp||_r = sqrt(sum over a of [dc^2 + r^2 (dcx^2 + dcy^2 + dcz^2) + r^4 (dcxx^2 / 4 + dcyy^2 / 4 + dczz^2 / 4 +
 *     dcxy^2 + dcxz^2 + dcyz^2)]): each term's displacement at the subset's edge.
 *   Domain: the warped subset is not the affine image of a box, so the rule is conservative and closed-form.  Per axis a,
 *     B_a = r^2 (|cxx| / 2 + |cyy| / 2 + |czz| / 2 + |cxy| + |cxz| + |cyz|) of that component.  With the 8 corners of the affine part
 *     (p with its second-order terms set to zero), p is in the domain when floor(min corner_a - B_a) - lo >= 0 and
 *     floor(max corner_a + B_a) + hi <= n_a - 1 on every axis, (lo, hi) = (1, 2) for the cubic interpolations and (0, 1) for the
 *     trilinear one; fp64, a NaN is outside.  With zero second-order terms this is sift3d_icgn's rule.
 *   Status table and its order: sift3d_icgn's (5, 2, 4, 3, 6, 4, 1, 0).
 *   Precision: the position of a voxel is floor(q + c) + d, integers, plus the fp32 sum frac(q + c) + (F - I) d + the quadratic part;
 *     the sample T' is fp32 as in sift3d_icgn; the products SD^T T' (Rx, Ry, Rz times T' times xi') and their sums are fp64.
 * o->interpolation: 0 Keys, 1 trilinear, 2 cubic B-spline; tar_is_coefficients has the meaning and the checks of
 * sift3d_icgn_bspline and must be 0 unless interpolation is 2.  SIFT3D_ERR_ARG (before any device call): as sift3d_icgn with these
 * rules; m = 0 succeeds.  The call keeps 4224 bytes of scratch per POI on the device.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct sift3d_icgn2_result {
	double p[30];          /* (c cx cy cz cxx cyy czz cxy cxz cyz) of u, then v, then w */
	double zncc;
	double last_step;      /* ||dp||_r of the last computed step (0: none) */
	int iterations;        /* updates applied */
	int status;            /* sift3d_icgn's table */
	int reserved[2];
} sift3d_icgn2_result;
SIFT3D_STATIC_ASSERT(sizeof(sift3d_icgn2_result) == 272, "sift3d_icgn2_result must be 272 bytes");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_icgn2_result, zncc) == 240 && offsetof(sift3d_icgn2_result, last_step) == 248 &&
                     offsetof(sift3d_icgn2_result, iterations) == 256 && offsetof(sift3d_icgn2_result, status) == 260 &&
                     offsetof(sift3d_icgn2_result, reserved) == 264, "sift3d_icgn2_result field offsets");

/* host only: m rows of 30 initial parameters from m first-order results; a row with status 0 or 1 gives its 12 parameters and zero
 * second derivatives, any other status a NaN row (POI status 5).  SIFT3D_ERR_ARG: m < 0, or a NULL pointer with m > 0. */
int sift3d_icgn2_init_from_icgn(const sift3d_icgn_result *res, int m, double *init30);
/* m POIs (x, y, z int triples) refined between ref and tar; init30: m*30 or NULL (zero) */
int sift3d_icgn2(const float *ref, int rnx, int rny, int rnz, const float *tar, int tnx, int tny, int tnz, const int *points3, int m,
                 const double *init30, const sift3d_icgn_options *o, int tar_is_coefficients, int on_device, int device,
                 sift3d_icgn2_result *out, double *seconds);

/* ------------------------------------------------------------------------------------------------------------
 * ZNCC integer search: the zero-order initial guess of IC-GN where no local affine fit exists (no reference counterpart: the
 * exhaustive integer-voxel search of DIC / DVC codes).  The reference subset of a POI is slid over a window of the target and the
 * integer displacement with the highest zero-normalised cross-correlation is returned.  It uses no neighbouring POI.
 * Numerical contract (a tolerance contract like IC-GN's, not bit for bit; tests/zncc_search_ref.py restates it in NumPy fp64):
 *   Volumes: fp32, [z][y][x], as for sift3d_icgn; R and T may differ in size.  A POI q is an integer voxel (x, y, z) of R.
 *   Subset: q + [-r, r]^3, N = (2r+1)^3 voxels; Rm = mean of R over it; dR = sqrt(sum (R - Rm)^2).
 *   Candidates: c = g + e with e in [-s, s]^3, g the POI's guess (zero without guess3).  c is admissible when q + c - r >= 0 and
 *     q + c + r <= n - 1 on every axis of T; a guess component of magnitude above 2^24 makes every candidate inadmissible.  The test
 *     is made in 64-bit arithmetic: no int overflows, whatever g holds.
 *   Score of an admissible candidate: zncc(c) = sum (R - Rm)(T(x + c) - Tm) / (dR dT), Tm and dT = sqrt(sum (T - Tm)^2) the mean
 *     and the deviation of T over the shifted subset.  A candidate with dT = 0 to rounding -- IC-GN's rule, dT^2 <= 1e-10 sum (T - Rm)^2
 *     -- is skipped, not scored.  A non-finite sum skips the candidate too; the sums meant are the float32 and fp64 sums of the
 *     Precision paragraph, so a candidate whose float32 products overflow (voxels of T - Tc beyond about 1.8e19) is skipped, and a
 *     NaN or Inf voxel of T silences exactly the candidates whose subset holds it.
 *   Result: the scored candidate with the highest score; among candidates whose scores are equal in the kernel's own arithmetic the
 *     lowest index (ez, ey, ex), ex fastest, wins.  zncc_second: the best score among the scored candidates at Chebyshev distance
 *     > 1 from d (-2.0: none).  candidates: how many were scored.
 *   Status per POI (results of a successful call, not errors), checked in this order:
 *     2 subset outside R;  4 dR = 0 (or not finite);  3 no candidate scored -- these return d = g, zncc 0, zncc_second -2.0, candidates 0;
 *     0 otherwise: the best scored candidate.  A POI with status 2 reads no voxel of R; no voxel outside R or T is ever read.
 *   Precision: the sums of a candidate are formed on T - Tc (ZNCC does not change when T is shifted).  Tc is a voxel of T: over the
 *     subset of T at q + g clamped to [r, n - 1 - r] on every axis (the subset of the admissible candidate nearest to e = 0), the
 *     finite voxel nearest to the fp64 mean of the finite voxels, the lowest index (dz, dy, dx) among equals, and 0 when no voxel is
 *     finite.  It lies within one standard deviation of that subset's mean, so no single voxel -- a dead or hot detector voxel at
 *     q + g -- sets the level, T - Tc is exact on integer-valued data, and a T constant over the search region has dT = 0 exactly
 *     and no candidate is scored.  A NaN or Inf at q + g therefore only skips the candidates that see it.  Products and the sums
 *     along x are fp32 ((R - (float)Rm) and (T - Tc) rounded once), the sums over rows, planes and slabs fp64, reduced in a fixed
 *     order with no float atomics: two calls return the same bytes, and a POI's result does not depend on the other POIs of the call.
 * SIFT3D_ERR_ARG (checked before any device call): m < 0, a dimension < 1, subset_radius outside 2..16, search_radius outside 1..16,
 * a non-zero reserved word, NULL ref / tar / out, NULL points3 with m > 0; m = 0 succeeds.  SIFT3D_ERR_NO_DEVICE after that check when
 * no GPU is visible: there is no CPU fallback.  o may be NULL (defaults).  on_device != 0: ref, tar, points3 and guess3 are device
 * pointers on `device`, ordered behind the legacy default stream; out is host memory, filled by one copy at the end.  *seconds (may
 * be NULL): device time of the call (HIP events; the uploads of host inputs excluded).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct sift3d_search_options {
	int subset_radius;     /* r, 2..16, default 8 */
	int search_radius;     /* s, 1..16, default 8 */
	int reserved[6];       /* must be 0 */
} sift3d_search_options;
SIFT3D_STATIC_ASSERT(sizeof(sift3d_search_options) == 32, "sift3d_search_options must be 32 bytes");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_search_options, search_radius) == 4 && offsetof(sift3d_search_options, reserved) == 8,
                     "sift3d_search_options field offsets");

typedef struct sift3d_search_result {
	int d[3];              /* best integer displacement (du, dv, dw) = guess + e */
	int status;            /* the table above */
	double zncc;           /* at d */
	double zncc_second;    /* best score among the scored candidates at Chebyshev distance > 1 from d; -2.0 if there is none */
	int candidates;        /* candidates scored */
	int reserved[3];       /* 0 */
} sift3d_search_result;
SIFT3D_STATIC_ASSERT(sizeof(sift3d_search_result) == 48, "sift3d_search_result must be 48 bytes");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_search_result, status) == 12 && offsetof(sift3d_search_result, zncc) == 16 &&
                     offsetof(sift3d_search_result, zncc_second) == 24 && offsetof(sift3d_search_result, candidates) == 32 &&
                     offsetof(sift3d_search_result, reserved) == 36, "sift3d_search_result field offsets");

/* the defaults above; needs no GPU */
void sift3d_default_search_options(sift3d_search_options *o);
/* m POIs (x, y, z int triples) of ref searched in tar; guess3: m int triples (gx, gy, gz) or NULL (zero); out: m records */
int sift3d_zncc_search(const float *ref, int rnx, int rny, int rnz, const float *tar, int tnx, int tny, int tnz, const int *points3, int m,
                       const int *guess3, const sift3d_search_options *o, int on_device, int device, sift3d_search_result *out,
                       double *seconds);
/* host only: fills rows of init12 (m * 12) from the search results with status 0 as (du, 0, 0, 0, dv, 0, 0, 0, dw, 0, 0, 0);
 * only_missing != 0: only rows that hold a non-finite value are touched.  Rows whose search failed stay as they are.
 * SIFT3D_ERR_ARG: m < 0, or a NULL pointer with m > 0. */
int sift3d_icgn_init_from_search(const sift3d_search_result *res, int m, int only_missing, double *init12);

/* ------------------------------------------------------------------------------------------------------------
 * Strain fields from the refined displacements (no reference counterpart: the pointwise least-squares window of DIC / DVC codes).
 * A plane is fitted to the displacements of the POIs around each POI and the strain is formed from the fitted gradient.
 * Numerical contract (a tolerance contract like IC-GN's and the search's, not bit for bit; tests/strain_ref.py restates it in NumPy
 * fp64):
 *   Inputs: points3, m integer voxels (x, y, z) -- the array given to sift3d_icgn; disp3, m rows (u, v, w) in fp64; valid, m bytes
 *     (NULL: every POI is valid).  A POI contributes as a neighbour only if its byte is non-zero, its three displacements are finite
 *     and every coordinate has magnitude <= 2^24.  Duplicate points are allowed and each one counts.
 *   Neighbours of POI i: the contributing POIs j with |x_j - x_i| <= radius, |y_j - y_i| <= radius and |z_j - z_i| <= radius, in integer
 *     arithmetic: membership is exact.  POI i is its own neighbour if it contributes.  A POI that does not contribute still gets a
 *     result from its neighbours (this fills holes), except that a POI with a coordinate of magnitude above 2^24 gets status 2, no fit.
 *   Fit: d_j = q_j - q_i, n the neighbour count, u0 the displacement of the neighbour with the lowest index; every sum of
 *     displacements is formed on u - u0, so a constant field gives G = 0, E = 0, rms = 0 and disp = the constant, exactly.
 *     S1 = sum d, S2 = sum d d^T (sums of integers: exact), U_c = sum (u_c - u0_c), P_ca = sum (u_c - u0_c) d_a, all fp64.
 *     C_ab = S2_ab - S1_a S1_b / n;  B_ca = P_ca - S1_a U_c / n;  C = L L^T (3 x 3 Cholesky);  row c of G = C^-1 B_c;
 *     disp_c = u0_c + U_c / n - G_c . S1 / n;
 *     rms = sqrt(sum_j sum_c (u_c(j) - disp_c - G_c . d_j)^2 / (3 n)), from a second pass over the neighbours (not from squared sums).
 *   Strain: measure 0 Green-Lagrange E = (G + G^T + G^T G) / 2; measure 1 infinitesimal E = (G + G^T) / 2.  principal: the eigenvalues
 *     of E, descending (cyclic Jacobi, fp64).  equivalent = sqrt(2/3 dev(E) : dev(E)), the shear terms counted twice.
 *   Status per POI (results of a successful call, not errors), checked in this order:
 *     2 a coordinate out of range (neighbours 0);  1 n < min_neighbours;  4 degenerate window: a Cholesky pivot (c00, c11 - l10^2,
 *     c22 - l20^2 - l21^2) is <= 1e-9 x the largest diagonal entry of C, or NaN -- coplanar and collinear neighbours land here;
 *     0 otherwise.  A non-zero status zeroes every double and reports n.
 *   Determinism: no float atomics; the neighbours are visited in an order the input alone fixes (cells of a uniform grid, a cell's
 *     POIs in ascending index) and every fp64 sum is reduced in a fixed order: two calls on the same input return the same bytes.
 * SIFT3D_ERR_ARG (checked before any device call): m < 0, radius outside 1..4096, min_neighbours outside 4..1048576, measure outside
 * 0..1, a non-zero reserved word, NULL out, NULL points3 or disp3 with m > 0; m = 0 succeeds.  SIFT3D_ERR_NO_DEVICE after that check
 * when no GPU is visible: there is no CPU fallback.  o may be NULL (defaults).  on_device != 0: points3, disp3 and valid are device
 * pointers on `device`, ordered behind the legacy default stream; out is host memory, filled by one copy at the end.  *seconds (may
 * be NULL): device time of the call (HIP events; the uploads of host inputs excluded).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct sift3d_strain_options {
	int radius;            /* window half width in voxels (Chebyshev), 1..4096, default 16 */
	int min_neighbours;    /* 4..1048576, default 10 */
	int measure;           /* 0 Green-Lagrange (default), 1 infinitesimal */
	int reserved[5];       /* must be 0 */
} sift3d_strain_options;
SIFT3D_STATIC_ASSERT(sizeof(sift3d_strain_options) == 32, "sift3d_strain_options must be 32 bytes");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_strain_options, min_neighbours) == 4 && offsetof(sift3d_strain_options, measure) == 8 &&
                     offsetof(sift3d_strain_options, reserved) == 12, "sift3d_strain_options field offsets");

typedef struct sift3d_strain_result {
	double disp[3];        /* fitted displacement at the POI (the plane's constant term) */
	double G[9];           /* fitted displacement gradient, row-major: rows u v w, columns x y z */
	double E[6];           /* xx yy zz xy yz zx of the chosen measure */
	double principal[3];   /* eigenvalues of E, descending */
	double equivalent;     /* sqrt(2/3 dev(E):dev(E)) */
	double rms;            /* residual of the fit */
	int neighbours;        /* n */
	int status;            /* the table above */
} sift3d_strain_result;
SIFT3D_STATIC_ASSERT(sizeof(sift3d_strain_result) == 192, "sift3d_strain_result must be 192 bytes");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_strain_result, G) == 24 && offsetof(sift3d_strain_result, E) == 96 &&
                     offsetof(sift3d_strain_result, principal) == 144 && offsetof(sift3d_strain_result, equivalent) == 168 &&
                     offsetof(sift3d_strain_result, rms) == 176 && offsetof(sift3d_strain_result, neighbours) == 184 &&
                     offsetof(sift3d_strain_result, status) == 188, "sift3d_strain_result field offsets");

/* the defaults above; needs no GPU */
void sift3d_default_strain_options(sift3d_strain_options *o);
/* host only, no GPU: row i of disp3 = (p[0], p[4], p[8]) of res[i]; valid[i] = 1 iff (status is 0, or status is 1 and
 * accept_unconverged != 0), zncc >= zncc_min and the three values are finite.  SIFT3D_ERR_ARG: m < 0, a non-finite zncc_min, or a
 * NULL pointer with m > 0. */
int sift3d_strain_input_from_icgn(const sift3d_icgn_result *res, int m, double zncc_min, int accept_unconverged, double *disp3,
                                  unsigned char *valid);
/* the same from second-order results: row i of disp3 = (p[0], p[10], p[20]) of res[i] */
int sift3d_strain_input_from_icgn2(const sift3d_icgn2_result *res, int m, double zncc_min, int accept_unconverged, double *disp3,
                                   unsigned char *valid);
/* m POIs (x, y, z int triples), their displacements (m * 3) and validity bytes (m, or NULL); out: m records */
int sift3d_strain(const int *points3, const double *disp3, const unsigned char *valid, int m, const sift3d_strain_options *o, int on_device,
                  int device, sift3d_strain_result *out, double *seconds);

/* ------------------------------------------------------------------------------------------------------------
 * Outlier validation of the displacement field: the normalised median test (Westerweel & Scarano 2005) for scattered 3-D POIs (no
 * reference counterpart).  The step between IC-GN and strain: a POI whose IC-GN converged on the wrong correlation peak has status 0
 * and a respectable ZNCC, and would spoil the plane fit of every POI within the strain window.  Its vector is compared with the
 * median of its neighbours' vectors, the difference scaled by their median absolute deviation (MAD) plus a noise floor.
 * Numerical contract (bit for bit: every step is one correctly rounded fp64 operation and nothing is summed over neighbours;
 * tests/validate_ref.py restates it in NumPy):
 *   Inputs: points3, disp3, valid as for sift3d_strain; grad9 (may be NULL): m rows of the POIs' own displacement gradients,
 *     row-major: rows u v w, columns x y z (IC-GN's p[1..3], p[5..7], p[9..11]).  A POI contributes under sift3d_strain's rule
 *     (non-zero valid byte, three finite displacements, every |coordinate| <= 2^24) and, with grad9 given, nine finite gradients.
 *   Neighbours of POI i: the contributing POIs j != i within `radius` of it (integer Chebyshev distance, exact); duplicates count, so
 *     a duplicate of POI i at another index is its neighbour, POI i itself never is.
 *   Neighbour j's estimate at POI i: e_c = u_c(j) without grad9; with it e_c = u_c(j) + ((G_c0 dx + G_c1 dy) + G_c2 dz), G row c of
 *     POI j's gradient and d = q_i - q_j as doubles, in this association and not fused.
 *   Statistics over a neighbour set N, n = |N|, per component c: median_c the exact order statistic of e_c (n odd: the middle value;
 *     n even: 0.5 * (lo + hi) of the two middle values); mad_c the same median of |e_c - median_c|;
 *     score = max_c |u_c(i) - median_c| / (mad_c + eps).  -0 and +0 are one value.  The result depends neither on the order of the
 *     neighbours nor on the order of the POIs.
 *   Passes: F_0 is empty.  In pass p = 1..passes every contributing POI i not in F_(p-1) is scored against N = {neighbours not in
 *     F_(p-1)}; all POIs of a pass read the flags of the pass before.  n >= min_neighbours and score > threshold: i joins F_p with
 *     pass = p.  Flags are never withdrawn.
 *   Report: after the last pass every POI gets a record from N built with the final F.  Status, checked in this order:
 *     2 a coordinate out of range (neighbours 0, the doubles 0);  1 n < min_neighbours (the doubles 0, n reported);  3 the POI does
 *     not contribute: median and mad are reported, score is 0 and the POI is never flagged -- the value that fills a hole;
 *     0 the POI was tested: score is its score against the final set.
 *     flagged and pass come from the passes and are authoritative: the final score of an unflagged POI may end above the threshold
 *     (its neighbourhood lost members in the last pass) and the POI stays unflagged.  A flagged POI whose final n is below the minimum
 *     keeps flagged = 1 with status 1.
 *   Determinism: no float atomics and no reductions in floating point: two calls return the same bytes.
 * SIFT3D_ERR_ARG (checked before any device call): m < 0, radius outside 1..4096, min_neighbours outside 3..1048576, passes outside
 * 1..8, a threshold or eps that is not finite and > 0, a non-zero reserved word, NULL out, NULL points3 or disp3 with m > 0; m = 0
 * succeeds.  SIFT3D_ERR_NO_DEVICE after that check when no GPU is visible: there is no CPU fallback.  o may be NULL (defaults).
 * on_device != 0: points3, disp3, grad9 and valid are device pointers on `device`, ordered behind the legacy default stream; out is
 * host memory, filled by one copy at the end.  *seconds (may be NULL): device time of the call (HIP events; uploads excluded).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct sift3d_validate_options {
	int radius;            /* window half width in voxels (Chebyshev), 1..4096, default 16 */
	int min_neighbours;    /* fewest neighbours a tested POI may have, 3..1048576, default 6 */
	int passes;            /* 1..8, default 2 */
	int reserved0;         /* must be 0 */
	double threshold;      /* finite, > 0, default 2.0: a score above it flags the POI */
	double eps;            /* finite, > 0, default 0.1: noise floor in voxels added to the MAD */
	int reserved[4];       /* must be 0 */
} sift3d_validate_options;
SIFT3D_STATIC_ASSERT(sizeof(sift3d_validate_options) == 48, "sift3d_validate_options must be 48 bytes");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_validate_options, min_neighbours) == 4 && offsetof(sift3d_validate_options, passes) == 8 &&
                     offsetof(sift3d_validate_options, reserved0) == 12 && offsetof(sift3d_validate_options, threshold) == 16 &&
                     offsetof(sift3d_validate_options, eps) == 24 && offsetof(sift3d_validate_options, reserved) == 32,
                     "sift3d_validate_options field offsets");

typedef struct sift3d_validate_result {
	double median[3];      /* of the neighbours' estimates at the POI, per component */
	double mad[3];         /* median absolute deviation of the same */
	double score;          /* max_c |u_c - median_c| / (mad_c + eps) against the final set; 0 unless status is 0 */
	int neighbours;        /* n of the final set */
	int status;            /* the table above */
	int flagged;           /* 1: an outlier (authoritative, from the passes) */
	int pass;              /* the pass that flagged it, 0 if none */
} sift3d_validate_result;
SIFT3D_STATIC_ASSERT(sizeof(sift3d_validate_result) == 72, "sift3d_validate_result must be 72 bytes");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_validate_result, mad) == 24 && offsetof(sift3d_validate_result, score) == 48 &&
                     offsetof(sift3d_validate_result, neighbours) == 56 && offsetof(sift3d_validate_result, status) == 60 &&
                     offsetof(sift3d_validate_result, flagged) == 64 && offsetof(sift3d_validate_result, pass) == 68,
                     "sift3d_validate_result field offsets");

/* the defaults above; needs no GPU */
void sift3d_default_validate_options(sift3d_validate_options *o);
/* host only, no GPU: sift3d_strain_input_from_icgn (the same disp3 and valid, by the same rule) and row i of grad9 = p[1..3], p[5..7],
 * p[9..11] of res[i]; grad9 may be NULL (not wanted).  SIFT3D_ERR_ARG as there. */
int sift3d_validate_input_from_icgn(const sift3d_icgn_result *res, int m, double zncc_min, int accept_unconverged, double *disp3,
                                    double *grad9, unsigned char *valid);
/* the same from second-order results: disp3 = (p[0], p[10], p[20]), grad9 = the first derivatives p[1..3], p[11..13], p[21..23] */
int sift3d_validate_input_from_icgn2(const sift3d_icgn2_result *res, int m, double zncc_min, int accept_unconverged, double *disp3,
                                     double *grad9, unsigned char *valid);
/* m POIs (x, y, z int triples), their displacements (m * 3), gradients (m * 9, or NULL) and validity bytes (m, or NULL); out: m records */
int sift3d_validate_displacements(const int *points3, const double *disp3, const double *grad9, const unsigned char *valid, int m,
                                  const sift3d_validate_options *o, int on_device, int device, sift3d_validate_result *out, double *seconds);
/* host only: valid_out[i] = 1 iff (valid_in is NULL or valid_in[i] != 0), val[i].status == 0 and val[i].flagged == 0 -- the bytes to
 * hand to sift3d_strain.  valid_out may be valid_in.  SIFT3D_ERR_ARG: m < 0, or NULL val / valid_out with m > 0. */
int sift3d_validate_keep(const sift3d_validate_result *val, const unsigned char *valid_in, int m, unsigned char *valid_out);
/* host only: the rows of init12 (m * 12) whose record is flagged with status 0, or has status 3, become (median_u, 0, 0, 0, median_v,
 * 0, 0, 0, median_w, 0, 0, 0): the neighbours' median as the start of a second sift3d_icgn.  Every other row stays as it is.
 * *count (may be NULL): rows written.  SIFT3D_ERR_ARG: m < 0, or NULL val / init12 with m > 0. */
int sift3d_icgn_init_from_validation(const sift3d_validate_result *val, int m, double *init12, int *count);

/* ------------------------------------------------------------------------------------------------------------
 * Evaluating the displacement field at any position (no reference counterpart: the moving least squares of scattered-data codes).
 * Every other result lives at the integer POIs of one call; this is the field at a real-valued position: a plane fitted to the
 * displacements of the POIs around the query, weighted so that the value moves continuously with the query.  It is what a load
 * series with an updated reference needs (the total at a reference POI p is u_A(p) + u_B(p + u_A(p)), and p + u_A(p) is no POI of
 * step B), what seeds a denser POI grid from a coarse one, and what samples the field on a lattice.
 * Numerical contract (a tolerance contract like sift3d_strain's, not bit for bit; tests/field_ref.py restates it in NumPy fp64):
 *   Inputs: points3, disp3, valid as for sift3d_strain, and a POI contributes under its rule: a non-zero valid byte (NULL: all),
 *     three finite displacements, every |coordinate| <= 2^24.  Duplicates each count.  queries3: nq rows (x, y, z) in fp64.
 *   Offsets: d_a = (double)q_j,a - x_a, one rounded subtraction, of contributing POI j from the query x.
 *   Members of query x: the contributing POIs with fabs(d_a) <= (double)radius on all three axes.
 *   Weights: weighting 0: w = 1.  Weighting 1 (tensor biweight): t_a = d_a / radius, f_a = 1 - t_a * t_a, g_a = f_a * f_a,
 *     w = (g_0 * g_1) * g_2.  A member on a face of the window has w = 0 exactly.  neighbours, sides and every sum count the members
 *     with w > 0 only.  sides: bit 2a is set when a counted member has d_a <= 0, bit 2a + 1 when one has d_a >= 0 (63: the query
 *     has neighbours on both sides of every axis).
 *   Fit: u0 is the displacement of the counted member with the lowest index and every sum of displacements is formed on u - u0.
 *     W = sum w;  S1 = sum w d;  S2 = sum w d d^T;  U_c = sum w (u_c - u0_c);  P_ca = sum w (u_c - u0_c) d_a, all fp64;
 *     C = S2 - S1 S1^T / W;  B_ca = P_ca - S1_a U_c / W;  C = L L^T (3 x 3 Cholesky, sift3d_strain's pivot rule: a pivot <= 1e-9 x
 *     the largest diagonal entry of C, or NaN, is a degenerate window);  row c of G = C^-1 B_c;
 *     disp_c = u0_c + U_c / W - G_c . S1 / W;
 *     rms = sqrt(sum w sum_c (u_c - disp_c - G_c . d)^2 / (3 W)), from a second pass over the members.
 *     With weighting 0 this is sift3d_strain's fit with n in place of W.  A constant field returns the constant, G = 0 and rms = 0
 *     exactly.
 *   Status per query (results of a successful call, not errors), checked in this order:
 *     2 a query coordinate is non-finite or beyond 2^24 in magnitude (neighbours and sides 0);  1 neighbours < min_neighbours;
 *     5 require_enclosed is set and sides != 63;  4 degenerate window;  0 otherwise.
 *     A non-zero status zeroes every double and still reports neighbours and sides.
 *   Determinism: no float atomics; the members are visited in the order of the POI index (cells of a uniform grid, a cell's POIs
 *     in ascending index) and every fp64 sum is reduced in a fixed order: two calls on the same input return the same bytes.
 * SIFT3D_ERR_ARG (checked before any device call): m < 0 or nq < 0, radius outside 1..4095, min_neighbours outside 4..1048576,
 * weighting or require_enclosed outside 0..1, a non-zero reserved word, NULL out or queries3 with nq > 0, NULL points3 or disp3 with
 * m > 0.  SIFT3D_ERR_NO_DEVICE after that check when no GPU is visible: there is no CPU fallback.  nq = 0 succeeds; m = 0 with
 * nq > 0 succeeds with status 1 at every query whose coordinates are in range.  o may be NULL (defaults).  on_device != 0: points3,
 * disp3, valid and queries3 are device pointers on `device`, ordered behind the legacy default stream; out is host memory, filled
 * by one copy at the end.  *seconds (may be NULL): device time of the call (HIP events; the uploads of host inputs excluded).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct sift3d_field_options {
	int radius;            /* window half width in voxels (Chebyshev), 1..4095, default 16 */
	int min_neighbours;    /* 4..1048576, default 10 */
	int weighting;         /* 1 (default): tensor biweight; 0: uniform */
	int require_enclosed;  /* 1 (default): status 5 unless the query has neighbours on both sides of every axis */
	int reserved[4];       /* must be 0 */
} sift3d_field_options;
SIFT3D_STATIC_ASSERT(sizeof(sift3d_field_options) == 32, "sift3d_field_options must be 32 bytes");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_field_options, min_neighbours) == 4 && offsetof(sift3d_field_options, weighting) == 8 &&
                     offsetof(sift3d_field_options, require_enclosed) == 12 && offsetof(sift3d_field_options, reserved) == 16,
                     "sift3d_field_options field offsets");

typedef struct sift3d_field_result {
	double disp[3];        /* the field at the query (the plane's constant term) */
	double G[9];           /* its gradient there, row-major: rows u v w, columns x y z */
	double rms;            /* weighted residual of the fit */
	double wsum;           /* W, the sum of the weights */
	int neighbours;        /* members with weight > 0 */
	int sides;             /* bit 2a: a member with d_a <= 0, bit 2a + 1: one with d_a >= 0 */
	int status;            /* the table above */
	int reserved;          /* 0 */
} sift3d_field_result;
SIFT3D_STATIC_ASSERT(sizeof(sift3d_field_result) == 128, "sift3d_field_result must be 128 bytes");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_field_result, G) == 24 && offsetof(sift3d_field_result, rms) == 96 &&
                     offsetof(sift3d_field_result, wsum) == 104 && offsetof(sift3d_field_result, neighbours) == 112 &&
                     offsetof(sift3d_field_result, sides) == 116 && offsetof(sift3d_field_result, status) == 120 &&
                     offsetof(sift3d_field_result, reserved) == 124, "sift3d_field_result field offsets");

/* the defaults above; needs no GPU */
void sift3d_default_field_options(sift3d_field_options *o);
/* m POIs (x, y, z int triples), their displacements (m * 3) and validity bytes (m, or NULL); nq queries (x, y, z doubles); out: nq
 * records */
int sift3d_field_eval(const int *points3, const double *disp3, const unsigned char *valid, int m, const double *queries3, int nq,
                      const sift3d_field_options *o, int on_device, int device, sift3d_field_result *out, double *seconds);
/* host only, no GPU: the positions the POIs moved to, x = (double)p + u per component -- the queries of the next load step.  The
 * result is non-finite where u is, and such a query gets status 2.  SIFT3D_ERR_ARG: m < 0, or a NULL pointer with m > 0. */
int sift3d_field_queries_from_displacements(const int *points3, const double *disp3, int m, double *queries3);
/* host only: row i of disp3 = res[i].disp, of grad9 = res[i].G, valid[i] = (res[i].status == 0); grad9 and valid may be NULL (not
 * wanted).  SIFT3D_ERR_ARG: n < 0, or NULL res / disp3 with n > 0. */
int sift3d_field_unpack(const sift3d_field_result *res, int n, double *disp3, double *grad9, unsigned char *valid);
/* host only: step A's result at its POIs (dispA3, gradA9 or NULL, validA or NULL: all valid) and step B's field evaluated where those
 * POIs moved to (atB) -> the total in step A's frame: disp = u_A + u_B and, with gradA9, grad = (G_A + G_B) + G_B G_A (from
 * F = F_B F_A with F = I + G), an entry of the product formed as (a * b + c * d) + e * f.  valid[i] = (validA is NULL or validA[i] != 0)
 * and atB[i].status == 0; the rows of an invalid POI are zero.  grad9 and valid may be NULL (not wanted).  SIFT3D_ERR_ARG: m < 0,
 * NULL dispA3 / atB / disp3 with m > 0, or a non-NULL grad9 with a NULL gradA9. */
int sift3d_compose_displacements(const double *dispA3, const double *gradA9, const unsigned char *validA, const sift3d_field_result *atB,
                                 int m, double *disp3, double *grad9, unsigned char *valid);
/* host only: row i of init12 (m * 12) becomes (u, G00, G01, G02, v, G10, G11, G12, w, G20, G21, G22) of row i of disp3 and grad9 (NULL:
 * a zero gradient): the start of sift3d_icgn from a measured field.  only_valid != 0: only the rows whose valid byte is set are
 * written (valid NULL: all) and the others stay as they are; only_valid == 0: every row is written.  *count (may be NULL): rows
 * written.  SIFT3D_ERR_ARG: m < 0, or NULL disp3 / init12 with m > 0. */
int sift3d_icgn_init_from_field(const double *disp3, const double *grad9, const unsigned char *valid, int m, int only_valid, double *init12,
                                int *count);

/* ------------------------------------------------------------------------------------------------------------
 * Subset screening: the step in front of IC-GN (no reference counterpart: the SSSIG rule of DIC / DVC codes, Pan et al. 2008,
 * Var(u) ~ 2 sigma_noise^2 / SSSIG_x).  Per POI it forms the texture sums of the subset -- the cube of voxels IC-GN would match -- at
 * growing radius and reports the smallest radius at which the sum of squared intensity gradients reaches a threshold, or that no
 * radius does: a subset in air, in a pore or in a phase with texture along one direction only cannot be correlated.
 * Numerical contract (tests/subset_ref.py restates it in NumPy fp64):
 *   Volume and POIs: those of sift3d_icgn: fp32 [z][y][x], a POI q an integer voxel (x, y, z) of R.
 *   Gradient: IC-GN's, fp32 g_x = 0.5f * (R[x+1] - R[x-1]) (likewise y, z), widened to double; every product and sum is fp64.
 *   Cube of radius rho: q + [-rho, rho]^3, N = (2 rho + 1)^3 voxels.  It is feasible when the cube plus a 1-voxel margin lies in R
 *     (IC-GN's status-2 rule).  feasible = rho_f: the largest rho <= r_max that is, computed in 64-bit arithmetic for any int q.
 *   Sums over a cube: Rc = R[q] is the shift and a = (double)R - (double)Rc (exact);  S = sum a;  Q = sum a^2;
 *     mean = (double)Rc + S / N;  dR = sqrt(v) with v = Q - S * S / N and v < 0 replaced by 0 (a NaN stays);
 *     G_ab = sum g_a g_b (xx yy zz xy xz yz);  material = the count of voxels with (double)R >= level.
 *     The operations in these formulas are single correctly rounded ones (the library is built with -ffp-contract=off).
 *   Eigenvalues: eig = those of G by cyclic Jacobi in fp64 (8 sweeps over the planes (0,1) (0,2) (1,2), as for sift3d_strain's
 *     principal), descending: the largest, trace - largest - smallest, the smallest.  Where an entry of G is not finite eig is NaN.
 *   Criterion: c(rho) = min(Gxx, Gyy, Gzz) (criterion 0, the per-axis SSSIG) or eig[2] (criterion 1); where an entry of G is not
 *     finite c(rho) is NaN under either.
 *   Selection: the reported radius is the smallest rho in [r_min, rho_f] whose c(rho) is finite and >= threshold; if there is none
 *     the record is that of rho_f with status 1.
 *   Status per POI (results of a successful call, not errors), checked in this order:
 *     2 the cube of r_min plus its margin is outside R: no voxel is read; the doubles, radius, feasible and material are 0;
 *     1 no radius qualifies;  3 a radius qualifies but (double)material < fraction_min * (double)N at that radius (the record is
 *     that radius's);  0 otherwise.
 *   Reach of a non-finite voxel: exactly the records whose cube or axial margin holds it.  A cube voxel's six axial neighbours are
 *     read; the edges and corners of the margin shell are not.  A NaN there makes c(rho) NaN, an Inf or a difference that overflows
 *     fp32 makes an entry of G non-finite: such a radius never qualifies.  A NaN or Inf at q itself reaches every sum through Rc.
 *   Determinism and bounds: no float atomics, every sum has a fixed order (the cube of r_min as one block, then the Chebyshev shells
 *     k = max(|dx|, |dy|, |dz|) outward, each added to the running totals); two calls return the same bytes; a POI's record does
 *     not depend on the other POIs of the call or on their order; no voxel outside R is ever read.
 *   Consequences: for integer-valued R (what 8 / 16-bit CT gives; sums below 2^53) S, Q and G are exact whatever the order, so
 *     mean, dR, G, material, radius and status equal the restatement bit for bit.  Scaling R by 2^e scales G by 2^(2e) bit for bit.
 *     A constant R gives all-zero sums exactly.  G, dR and mean at radius r are sift3d_icgn's H[0][0], H[4][4], H[8][8], H[0][4],
 *     H[0][8], H[4][8], dR and Rm at that r (to the rounding of the sums: IC-GN forms dR in two passes).
 * SIFT3D_ERR_ARG (checked before any device call): m < 0, a dimension < 1, r_min outside 2..32, r_max outside r_min..32, criterion
 * outside 0..1, a threshold that is not finite and >= 0, a NaN level, fraction_min outside 0..1 (or NaN), a non-zero reserved word,
 * NULL ref / out, NULL points3 with m > 0; m = 0 succeeds.  SIFT3D_ERR_NO_DEVICE after that check when no GPU is visible: there is
 * no CPU fallback.  o may be NULL (defaults).  on_device != 0: ref and points3 are device pointers on `device`, ordered behind the
 * legacy default stream; out is host memory, filled by one copy at the end.  *seconds (may be NULL): device time of the call (HIP
 * events; the uploads of host inputs excluded).
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct sift3d_subset_options {
	int r_min;             /* 2..32, default 8 */
	int r_max;             /* r_min..32, default 16 */
	int criterion;         /* 0 (default): min(Gxx, Gyy, Gzz), the per-axis SSSIG;  1: the smallest eigenvalue of G */
	int reserved0;         /* must be 0 */
	double threshold;      /* finite, >= 0, default 0 (accepts r_min everywhere: the caller sets it, 2 sigma_noise^2 / sigma_u^2) */
	double level;          /* not NaN, default -INFINITY: a voxel is "material" when (double)R >= level */
	double fraction_min;   /* 0..1, default 0 */
	int reserved[2];       /* must be 0 */
} sift3d_subset_options;
SIFT3D_STATIC_ASSERT(sizeof(sift3d_subset_options) == 48, "sift3d_subset_options must be 48 bytes");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_subset_options, r_max) == 4 && offsetof(sift3d_subset_options, criterion) == 8 &&
                     offsetof(sift3d_subset_options, reserved0) == 12 && offsetof(sift3d_subset_options, threshold) == 16 &&
                     offsetof(sift3d_subset_options, level) == 24 && offsetof(sift3d_subset_options, fraction_min) == 32 &&
                     offsetof(sift3d_subset_options, reserved) == 40, "sift3d_subset_options field offsets");

typedef struct sift3d_subset_result {
	double mean;           /* Rm over the reported cube */
	double dR;             /* sqrt(sum (R - Rm)^2) */
	double G[6];           /* xx yy zz xy xz yz: sums of products of the fp32 central differences */
	double eig[3];         /* eigenvalues of G, descending */
	int radius;            /* the reported radius */
	int status;            /* the table above */
	int feasible;          /* largest rho <= r_max whose cube + 1-voxel margin lies in R (0 with status 2) */
	int material;          /* voxels of the reported cube with R >= level */
} sift3d_subset_result;
SIFT3D_STATIC_ASSERT(sizeof(sift3d_subset_result) == 104, "sift3d_subset_result must be 104 bytes");
SIFT3D_STATIC_ASSERT(offsetof(sift3d_subset_result, dR) == 8 && offsetof(sift3d_subset_result, G) == 16 &&
                     offsetof(sift3d_subset_result, eig) == 64 && offsetof(sift3d_subset_result, radius) == 88 &&
                     offsetof(sift3d_subset_result, status) == 92 && offsetof(sift3d_subset_result, feasible) == 96 &&
                     offsetof(sift3d_subset_result, material) == 100, "sift3d_subset_result field offsets");

/* the defaults above; needs no GPU */
void sift3d_default_subset_options(sift3d_subset_options *o);
/* m POIs (x, y, z int triples) of ref screened; out: m records */
int sift3d_subset_quality(const float *ref, int nx, int ny, int nz, const int *points3, int m, const sift3d_subset_options *o,
                          int on_device, int device, sift3d_subset_result *out, double *seconds);
/* host only: the status-0 records grouped by radius, for one sift3d_icgn call per non-empty group with that group's radius.
 * order (m ints): the indices of the status-0 records by ascending radius, ascending index within a radius; offsets
 * (r_max - r_min + 2 ints): group g = radius r_min + g is order[offsets[g] .. offsets[g + 1]); *count: how many records were listed.
 * SIFT3D_ERR_ARG: m < 0, r_min outside 2..32, r_max outside r_min..32, a NULL pointer with m > 0 (with m = 0 offsets and count are
 * filled where given), or a status-0 record whose radius lies outside r_min..r_max. */
int sift3d_subset_group_by_radius(const sift3d_subset_result *res, int m, int r_min, int r_max, int *order, int *offsets, int *count);

/* ------------------------------------------------------------------------------------------------------------
 * Masked IC-GN: subsets limited to a voxel mask of the reference (no reference counterpart: what DVC codes do at a specimen's surface,
 * at pores and cracks and where two bodies touch -- they correlate over "the voxels of the subset that are material").  A POI closer
 * than r to such an edge has a full cube [-r, r]^3 that holds air or the other body; sift3d_icgn converges there with a high zncc and
 * a displacement that is wrong by tenths of a voxel, and the screening can only reject the point (status 3).
 * Numerical contract (a tolerance contract like sift3d_icgn's; tests/icgn_mask_ref.py restates it in NumPy fp64):
 *   Mask: one unsigned char per voxel of R, in R's layout [z][y][x]; any non-zero byte is "in".
 *   Active voxel: it and its six face neighbours lie in R and are in the mask, so the central differences of R never straddle the
 *     mask's edge.  R's own boundary voxels are never active.
 *   sift3d_icgn_masked is sift3d_icgn (o->interpolation 0 or 1) or sift3d_icgn_bspline (2) with one change: every sum over the subset
 *     runs over the active voxels of the cube only -- Rm, dR, sum SD, sum SD^T R', H, the correction term of zncc and the sums of each
 *     pass (sum T', sum T'^2, sum R'T', sum SD^T T') -- in the same walk order, an inactive voxel being skipped, not multiplied by
 *     zero: neither R nor T is read there.  The active count n of the cube takes N's place in Rm, Tm and sum (T - Rm)^2.
 *   Everything else is sift3d_icgn's contract word for word: the 8-corner domain test of the full box, status 2 on the full cube plus
 *     its margin, Tc (T's voxel under the subset's centre, active or not), the update, the norm with r^2 and the status table.
 *   Status 7 (new): n == 0, or (double)n < (double)min_fraction * (double)N with N = (2r+1)^3 (the form of the screening's status-3
 *     rule).  Checked after 5 and 2 and before 4; returns the init as given, iterations 0, zncc 0.  A mask that leaves H not positive
 *     definite (fewer than 12 active voxels, or active voxels in one plane) gives status 4 as a flat subset does.
 *   active[i] (may be NULL): n of POI i; 0 with status 5 or 2, where no voxel is read.
 *   Consequences (tests/test_gpu_icgn_mask.py):
 *     (a) with a mask whose bytes are all non-zero every field of every record has the bits of sift3d_icgn / sift3d_icgn_bspline on
 *         the same inputs (n = N; the walk, the per-thread sums and the reduction are the unmasked kernel's);
 *     (b) R's values at voxels that are neither active nor a face neighbour of an active voxel, non-finite ones included, do not
 *         influence the result;
 *     (c) two calls return the same bytes;
 *     (d) a POI's record does not depend on the other POIs of the call.
 * o->interpolation: 0 Keys, 1 trilinear, 2 cubic B-spline; tar_is_coefficients as for sift3d_icgn2 (0 unless interpolation is 2).
 * SIFT3D_ERR_ARG (checked before any device call): sift3d_icgn's rules with these, a NULL mask, min_fraction outside 0..1 or NaN;
 * m = 0 succeeds.  SIFT3D_ERR_NO_DEVICE after that check when no GPU is visible: there is no CPU fallback.  on_device != 0: ref, tar,
 * mask, points3 and init12 are device pointers on `device`; out and active are host memory.  The call keeps one byte per voxel of R
 * (two for host inputs) and 4 bytes per POI on the device beside sift3d_icgn's scratch; *seconds includes the pass that marks the
 * active voxels.
 *
 * sift3d_mask_from_level: mask[i] = 1 where (double)vol[i] >= level, else 0 (a NaN voxel is 0): the screening's rule for `material`, so
 * the mask and sift3d_subset_quality's count agree.  SIFT3D_ERR_ARG (before any device call): NULL vol / mask, a dimension < 1, 2^39
 * voxels or more, a NaN level (+-INFINITY are levels).  on_device != 0: vol and mask are device pointers on `device`, ordered behind the
 * legacy default stream; otherwise both are host memory.  *seconds (may be NULL): device time of the kernel.
 * ------------------------------------------------------------------------------------------------------------ */
int sift3d_icgn_masked(const float *ref, int rnx, int rny, int rnz, const float *tar, int tnx, int tny, int tnz,
                       const unsigned char *mask /* rnx*rny*rnz */, const int *points3, int m, const double *init12,
                       const sift3d_icgn_options *o, float min_fraction /* 0..1 */, int tar_is_coefficients, int on_device, int device,
                       sift3d_icgn_result *out, int *active /* m, may be NULL */, double *seconds);
int sift3d_mask_from_level(const float *vol, int nx, int ny, int nz, double level, unsigned char *mask, int on_device, int device,
                           double *seconds);

/* ------------------------------------------------------------------------------------------------------------
 * Several bodies: connected-component labels of a mask, and the three window calls limited to a POI's own body (no reference
 * counterpart: what DVC codes for granular specimens do).  sift3d_strain, sift3d_validate_displacements and sift3d_field_eval take
 * every contributing POI of the window as a neighbour, whichever body it lies in: across a contact between two bodies that move
 * differently the plane fit reports a strain that is not there, the median test flags the correct vectors of the smaller body, and
 * the field is a blend of two motions.  The labels say which body a voxel and a POI belong to.
 *
 * sift3d_mask_label: the components of a byte mask (tests/label_ref.py restates it in NumPy).
 *   Layout [z][y][x], x fastest, as every volume here; any non-zero mask byte is "in".  labels[i] = 0 where mask[i] is 0.
 *   A component is a maximal set of in-voxels connected through faces (connectivity 6) or through faces, edges and corners (26).
 *   The kept components -- those of at least min_voxels voxels -- are numbered 1..*count in ascending order of their lowest linear
 *   voxel index (z * ny + y) * nx + x (scipy.ndimage.label's numbering); a voxel of a smaller component gets 0 and the component is
 *   neither counted nor numbered.
 *   Determinism: the output is a function of the input alone (integer atomics only): two calls return the same bytes.
 *   SIFT3D_ERR_ARG (checked before any device call): NULL mask, labels or count, a dimension < 1, nx * ny * nz >= 2^31 (linear
 *   indices are int), a connectivity other than 6 or 26, min_voxels < 1.  SIFT3D_ERR_NO_DEVICE after that check when no GPU is
 *   visible: there is no CPU fallback.  on_device != 0: mask and labels are device pointers on `device`, ordered behind the legacy
 *   default stream; otherwise both are host memory.  count is host memory either way.  *seconds (may be NULL): device time of the
 *   kernels (the copies excluded).
 *   Device memory: beside labels the call keeps 4 bytes per voxel and 4 bytes per 2048 voxels, and with host pointers 5 more bytes per
 *   voxel (the mask and the labels), in a block that grows with the largest call so far (a quarter of head room) and stays allocated
 *   for later calls.
 *
 * sift3d_labels_at_points: poi_label[i] = labels at voxel points3[i] (x, y, z), or 0 when that voxel lies outside the volume.
 *   on_device == 0: a host loop, no GPU needed.  on_device != 0: labels and points3 are device pointers on `device`, ordered behind
 *   the legacy default stream; poi_label is host memory either way, filled by one kernel and one copy.  SIFT3D_ERR_ARG: NULL labels,
 *   a dimension < 1, nx * ny * nz >= 2^31, m < 0, NULL points3 or poi_label with m > 0.
 *
 * sift3d_labels_at_positions: out_label[i] = labels at the voxel nearest to the fp32 position (x, y, z) = xyz[i * stride .. + 2], or 0
 *   outside the volume.  Per axis the position is in the volume iff -0.5 <= (double)x && (double)x < n_axis - 0.5, tested before the
 *   conversion (NaN and +-Inf fail the test); then i = (long long)floor((double)x + 0.5).  stride: floats between positions, >= 3;
 *   stride = 6 labels the reference positions of pairs6 directly.  on_device == 0: a host loop, no GPU needed.  on_device != 0:
 *   labels and xyz are device pointers on `device`, ordered behind the legacy default stream; out_label is host memory either way,
 *   filled by one kernel and one copy.  SIFT3D_ERR_ARG: NULL labels, a dimension < 1, nx * ny * nz >= 2^31, n < 0, stride < 3, NULL xyz
 *   or out_label with n > 0.
 *
 * The labelled window calls: sift3d_strain, sift3d_validate_displacements and sift3d_field_eval with one sentence added to each
 * contract.  POI j is a neighbour (strain, validation) or a member (field) of centre i only if it is one under the unlabelled rule
 * and label[j] == label[i] and that label is > 0; for a field query k, query_label[k] takes the place of label[i].  A centre or query
 * whose label is <= 0 has no neighbours: status 1 with neighbours 0 (and sides 0); the coordinate test, status 2, still comes first.
 * u0, "the neighbour with the lowest index", is taken among the neighbours so defined.  Everything else stands word for word: which
 * POIs contribute, hole filling (status 3), the passes of the median test, require_enclosed, the pivot rule, determinism.  With all
 * labels equal and positive a call returns the bytes of the unlabelled call.  A POI's record does not depend on the POIs of other
 * labels: the lanes of a wave share out the entries of the centre's label alone, so the other POIs' displacements, finite or not,
 * do not move a single fp64 sum -- as long as the bounding box of the contributing POIs, which places the cell grid and with it the
 * order of a window's entries, stays where it is (a validation record, which sums nothing, is independent without that).  label: m ints; query_label: nq ints; device pointers when on_device != 0.  SIFT3D_ERR_ARG: the unlabelled call's rules
 * with these, a NULL label, a NULL query_label with nq > 0.  A per-body mask for sift3d_icgn_masked is labels == L.
 *
 * sift3d_icgn_labelled: every POI correlated over its own body, in one call.  POI i is treated as sift3d_icgn_masked treats it under
 * the mask labels == labels[q_i].
 *   A voxel is active for POI i iff it and its six face neighbours lie in R and all seven carry the label L_i = labels[q_i], with
 *   L_i > 0.  With L_i <= 0 the POI has n = 0 and therefore status 7; statuses 5 and 2 still come first.  Any positive int is a label:
 *   the numbers need not be 1..count, so a watershed segmentation from elsewhere serves as well.
 *   Everything else is the masked call's text: the statuses, min_fraction, the three interpolations, tar_is_coefficients, determinism,
 *   the independence of a POI from the other POIs of the call, and R's values away from a POI's active voxels and their face
 *   neighbours not being read for it.
 *   Consequence (tests/test_gpu_icgn_labelled.py): for every label L, the records and the active counts of the POIs of L have the bits
 *   of one sift3d_icgn_masked call on those POIs with the byte mask labels == L; with one positive label everywhere, those of
 *   sift3d_icgn / sift3d_icgn_bspline.
 *   poi_label[i] (may be NULL) = L_i, or 0 when q_i lies outside R; active[i] (may be NULL) as in the masked call.
 * SIFT3D_ERR_ARG (checked before any device call): the masked call's rules with a NULL labels in the NULL mask's place, and
 * rnx * rny * rnz >= 2^31.  on_device != 0: ref, tar, labels, points3 and init12 are device pointers on `device`; out, active and
 * poi_label are host memory.  The call keeps 4 bytes per voxel of R (8 for host inputs) and 8 bytes per POI on the device beside
 * sift3d_icgn's scratch; *seconds includes the pass that writes the interior labels.  sift3d_icgn2, the search and the screening
 * stay unlabelled.
 * ------------------------------------------------------------------------------------------------------------ */
int sift3d_mask_label(const unsigned char *mask, int nx, int ny, int nz, int connectivity /* 6 or 26 */, int min_voxels /* >= 1 */,
                      int *labels /* nx*ny*nz */, int *count, int on_device, int device, double *seconds);
int sift3d_labels_at_points(const int *labels, int nx, int ny, int nz, const int *points3, int m, int *poi_label /* m, host */, int on_device,
                            int device);
int sift3d_labels_at_positions(const int *labels, int nx, int ny, int nz, const float *xyz /* fp32 */, int stride /* floats, >= 3 */, int n,
                               int *out_label /* n, host */, int on_device, int device);
int sift3d_icgn_labelled(const float *ref, int rnx, int rny, int rnz, const float *tar, int tnx, int tny, int tnz,
                         const int *labels /* rnx*rny*rnz */, const int *points3, int m, const double *init12,
                         const sift3d_icgn_options *o, float min_fraction, int tar_is_coefficients, int on_device, int device,
                         sift3d_icgn_result *out, int *active /* m, may be NULL */, int *poi_label /* m, may be NULL */, double *seconds);
int sift3d_strain_labelled(const int *points3, const double *disp3, const unsigned char *valid, const int *label /* m */, int m,
                           const sift3d_strain_options *o, int on_device, int device, sift3d_strain_result *out, double *seconds);
int sift3d_validate_displacements_labelled(const int *points3, const double *disp3, const double *grad9, const unsigned char *valid,
                                           const int *label /* m */, int m, const sift3d_validate_options *o, int on_device, int device,
                                           sift3d_validate_result *out, double *seconds);
int sift3d_field_eval_labelled(const int *points3, const double *disp3, const unsigned char *valid, const int *label /* m */, int m,
                               const double *queries3, const int *query_label /* nq */, int nq, const sift3d_field_options *o, int on_device,
                               int device, sift3d_field_result *out, double *seconds);

/* ------------------------------------------------------------------------------------------------------------
 * Bodies that touch: the distance transform of a mask and labels grown from its cores (no reference counterpart: the marker-based
 * separation of touching grains).  Grains that touch are one component of a threshold mask, so sift3d_mask_label returns one label for
 * all of them; sift3d_mask_split gives every grain that is wide enough to hold a core a label of its own.  tests/split_ref.py restates
 * both rules in NumPy.
 *
 * sift3d_mask_distance: the exact squared Euclidean distance of every in-voxel to the nearest out-voxel.
 *   Layout [z][y][x], x fastest; any non-zero mask byte is "in".  dist2[i] = 0 for an out-voxel.  For an in-voxel i, dist2[i] is the
 *   minimum over all out-voxels j of (xi - xj)^2 + (yi - yj)^2 + (zi - zj)^2, an exact integer.
 *   border = 1: the voxels just outside the volume (a coordinate of -1 or n on any axis) count as out-voxels, so an in-voxel on a face
 *   of the volume has dist2 = 1: what a specimen cut by the field of view needs.  border = 0: only the volume's own out-voxels count,
 *   and where there is none every in-voxel gets SIFT3D_DIST2_NONE.
 *   With border = 0 and at least one out-voxel the result is rint(scipy.ndimage.distance_transform_edt(mask) ** 2); with border = 1
 *   the same of the mask padded by one layer of zeros, cropped back.
 *   Determinism: the output is a function of the input alone (integer minima): two calls return the same bytes.
 *   SIFT3D_ERR_ARG (checked before any device call): NULL mask or dist2, a dimension < 1, nx * ny * nz >= 2^31,
 *   (nx + 1)^2 + (ny + 1)^2 + (nz + 1)^2 >= 2^31 (every distance fits an int), border outside 0..1.  SIFT3D_ERR_NO_DEVICE after that
 *   check when no GPU is visible: there is no CPU fallback.  on_device != 0: mask and dist2 are device pointers on `device`, ordered
 *   behind the legacy default stream; otherwise both are host memory.  *seconds (may be NULL): device time of the three kernels.
 *   Device memory: beside dist2 the call keeps 4 bytes per voxel, and with host pointers 5 more (the mask and dist2), in a block that
 *   grows with the largest call so far and stays allocated.
 *
 * sift3d_mask_from_distance: mask[i] = 1 where dist2[i] >= level2, else 0: with level2 >= 1 the exact erosion of the mask by the open
 *   ball of squared radius level2.  SIFT3D_ERR_ARG (before any device call): NULL dist2 / mask, a dimension < 1, 2^39 voxels or more.
 *   on_device, *seconds: as sift3d_mask_from_level.
 *
 * sift3d_distance_at_points: poi_dist2[i] = dist2 at voxel points3[i] (x, y, z), or 0 when that voxel lies outside the volume: the
 *   squared distance of a POI to the surface of its body, by which a caller drops or down-weights the POIs whose subset reaches across
 *   it.  Pointers, the host loop of on_device == 0 and SIFT3D_ERR_ARG: as sift3d_labels_at_points.
 *
 * sift3d_mask_split: labels of bodies that may touch.  The rule, with d = the transform and c = connectivity:
 *   1. d = sift3d_mask_distance(mask, border).
 *   2. Cores: L0 = sift3d_mask_label(d >= core_dist2, c, min_core_voxels), with that call's numbering (ascending lowest voxel of the
 *      core); info->cores is its count.
 *   3. Growth in synchronous rounds, from labels = L0.  In a round every in-voxel whose label was 0 at the start of the round looks at
 *      its 6 or 26 neighbours inside the volume whose label was > 0 at the start of the round; if there is one, the voxel takes the
 *      label of the neighbour with the largest d, and among neighbours of equal d the smallest label.  A labelled voxel never changes.
 *      The growth stops after the first round that labels nothing, or after max_rounds rounds (max_rounds > 0); info->rounds is the
 *      number of rounds that labelled at least one voxel.
 *   4. keep_unreached = 1: the in-voxels still at 0 are labelled by sift3d_mask_label(that set, c, min_voxels) and numbered
 *      cores + 1 ...; info->unreached_bodies is their count (0 with keep_unreached = 0).  A grain too small to hold a core keeps an
 *      identity when it stands alone; one that touches a grain with a core is absorbed by it.
 *   5. *count = cores + unreached_bodies; info->unlabelled = the in-voxels left at 0.  labels[i] = 0 for every out-voxel.
 *   Consequences (tests/test_split_cpu.py, tests/test_gpu_split.py): (a) with core_dist2 = 1, and min_core_voxels = 1 or
 *   keep_unreached = 0, labels and count are the bytes of sift3d_mask_label(mask, c, min_core_voxels) and rounds = 0; (b) two calls
 *   return the same bytes (no result depends on the order of execution: a round reads one volume and writes another); (c) the voxels of
 *   a label are connected under c; (d) two voxels with the same split label have the same sift3d_mask_label label: the split only
 *   refines; (e) the labels on the core voxels are L0's.
 *   Choosing core_dist2: above the squared half-width of the widest neck between two grains (or they share a core), and at most the
 *   squared inradius of the smallest grain to keep apart (or it holds no core).
 *   dist2 (may be NULL): the transform, as sift3d_mask_distance returns it.  info (may be NULL).
 *   SIFT3D_ERR_ARG (checked before any device call): sift3d_mask_distance's and sift3d_mask_label's rules, NULL o, labels or count,
 *   connectivity other than 6 or 26, core_dist2 < 1, min_core_voxels < 1, border outside 0..1, max_rounds < 0, keep_unreached outside
 *   0..1, min_voxels < 1.  SIFT3D_ERR_NO_DEVICE after that check when no GPU is visible.  on_device != 0: mask, labels and dist2 are
 *   device pointers on `device`, ordered behind the legacy default stream; otherwise host memory.  count and info are host memory.
 *   *seconds (may be NULL): device time from the first kernel to the last, the read-backs of the round counters included (one per eight
 *   rounds).  Device memory: beside labels 9 bytes per voxel and 4 bytes per 2048 voxels, 4 more per voxel when dist2 is NULL or host
 *   memory, and with host pointers 5 more (the mask and the labels).
 * ------------------------------------------------------------------------------------------------------------ */
#define SIFT3D_DIST2_NONE 2147483647
typedef struct {
	int connectivity;    /* 6 or 26: of the cores' components and of the growth                                  default 6  */
	int core_dist2;      /* >= 1: a core voxel has dist2 >= core_dist2                                           default 16 */
	int min_core_voxels; /* >= 1: smaller cores seed nothing                                                     default 1  */
	int border;          /* 0 or 1, as sift3d_mask_distance                                                      default 1  */
	int max_rounds;      /* >= 0: growth rounds at most; 0 = until a round labels nothing                        default 0  */
	int keep_unreached;  /* 0: in-voxels no core reaches stay 0; 1: their components become bodies too           default 1  */
	int min_voxels;      /* >= 1: size cut of those components                                                   default 1  */
} sift3d_split_options;
typedef struct {
	int cores, unreached_bodies, rounds, unlabelled;
} sift3d_split_info;
void sift3d_default_split_options(sift3d_split_options *o);
int sift3d_mask_distance(const unsigned char *mask, int nx, int ny, int nz, int border /* 0 or 1 */, int *dist2 /* nx*ny*nz */, int on_device,
                         int device, double *seconds);
int sift3d_mask_from_distance(const int *dist2, int nx, int ny, int nz, int level2, unsigned char *mask, int on_device, int device,
                              double *seconds);
int sift3d_distance_at_points(const int *dist2, int nx, int ny, int nz, const int *points3, int m, int *poi_dist2 /* m, host */, int on_device,
                              int device);
int sift3d_mask_split(const unsigned char *mask, int nx, int ny, int nz, const sift3d_split_options *o, int *labels /* nx*ny*nz */, int *count,
                      int *dist2 /* nx*ny*nz, may be NULL */, sift3d_split_info *info /* may be NULL */, int on_device, int device,
                      double *seconds);

/* Test hooks, rare-path counters and the unit-level debug entry points live in include/sift3d_hip_test.h: this header is the
 * product boundary only. */
const char *sift3d_error_string(int code);
const char *sift3d_last_error(void); /* thread-local detail of the last failure */

#ifdef __cplusplus
}
#endif
#endif
