/*
 * lt_abi.h — C ABI of the MI355X LandTrendr analysis engine (land_trendr_amd/liblt_hip.so).
 *
 * Drop-in boundary for the reference's per-pixel hot path. The reference is pure Python and binds
 * no native code; this ABI replaces, per batched tile of pixels:
 *   - utils.analyze(pix_datas, line_cost, target_date)        /root/reference/utils.py:735-789
 *       pick_winners :491-521, dicts2timeseries :523-532, despike :556-582,
 *       timeseries2int_series :534-554, least_squares :584-598, segmented_least_squares :600-631,
 *       find_segments :633-644, vertices2eqns :646-669, eqns2fitted_points :682-722
 *   - utils.change_labeling(trendline, label_rules)          /root/reference/utils.py:795-820
 *       Trendline.parse_disturbances / match_rule             /root/reference/classes.py:156-232
 *   - the per-pixel loop of MRLandTrendrJob.analysis_reducer  /root/reference/mr_land_trendr_job.py:83-126
 *     (one call per grid point there; one call per pixel tile here).
 * The Python host (land_trendr_amd/utils.py, classes.py) binds it with ctypes; INTEGRATION.md shows
 * the binding. Plain C types only: no torch types cross this boundary.
 *
 * Memory: the caller owns every buffer. lt_tile_in / lt_tile_out pointers are DEVICE pointers
 * (hipMalloc or torch tensors on the context's device); lt_scene / lt_params are HOST structs that
 * the call copies. Any lt_tile_out pointer may be NULL: that field is not written.
 * Layout: pixel-major structure of arrays. Plane q of a field starts at base + q*stride, the pixel
 * index runs fastest, so lane i of a wavefront touches element i of a plane (coalesced).
 */
#ifndef LT_ABI_H
#define LT_ABI_H
#ifndef __HIPCC_RTC__  /* hiprtc (the JIT kernels) brings its own */
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define LT_ABI_VERSION 8
#define LT_MAX_YEARS 64   /* distinct calendar years per scene (T <= 40 in every bench config;
                             checked up to 64 consecutive years with up to LT_MAX_RULES rules and
                             LT_MAX_OBS observations: tests/test_gpu_wide.py, test_wide_host.py) */
#define LT_MAX_OBS 1024   /* observations per scene (K*T) */
#define LT_MAX_RULES 16
#define LT_NODATA (-99)   /* settings.py:16 */
#define LT_MAX_TILE_PIX (1LL << 28) /* pixels per analyzed tile (lt_tile_in.n_pix)           */
#define LT_MAX_ZONES 65536          /* zones of a zonal table (lt_zonal_stats)                */

/* Per-pixel status bits (lt_tile_out.status). Non-zero = the reference raises for this pixel. */
enum {
  LT_ST_OK = 0,
  LT_ST_EMPTY = 1,              /* no valid observation: reference IndexError (utils.py:569)     */
  LT_ST_SINGLE_YEAR = 2,        /* T == 1: reference ValueError in despike (utils.py:582)        */
  LT_ST_PRE_THRESHOLD_ATTR = 4, /* pre_threshold in reference mode: AttributeError (classes.py:207) */
  LT_ST_FEB29 = 8,              /* Feb-29 target in a non-leap year: ValueError (utils.py:511)   */
  LT_ST_NUMERIC = 16            /* LAPACK path not emulated (rank < 2 / DLASCL rescaling)        */
};

/* Return codes of the API functions. */
enum {
  LT_OK = 0,
  LT_ERR_ARG = -1,
  LT_ERR_HIP = -2,
  LT_ERR_JIT = -3,
  LT_ERR_LIMIT = -4
};

enum { LT_CT_NONE = 0, LT_CT_FD = 1, LT_CT_GD = 2, LT_CT_LD = 3 };          /* classes.py:44-47 */
enum { LT_Q_UNSET = 0, LT_Q_EQ = 1, LT_Q_LE = 2, LT_Q_GE = 3, LT_Q_GT = 4, LT_Q_LT = 5,
       LT_Q_OTHER = 9 /* set, but a qualifier match_rule ignores (classes.py:190-211) */ };
enum { LT_PRE_REFERENCE = 0, LT_PRE_DOCUMENTED = 1 };                      /* SURVEY App. B #1 */

/* One validated LabelRule (classes.py:32-64). The host performs the validation. */
typedef struct {
  int32_t change_type;   /* LT_CT_*                                  */
  int32_t onset_op;      /* LT_Q_UNSET / EQ / LE / GE / OTHER        */
  int32_t duration_op;   /* LT_Q_UNSET / GT / LT / OTHER             */
  int32_t pre_op;        /* LT_Q_UNSET / GT / LT / OTHER             */
  double onset_val;
  double duration_val;
  double pre_val;
  int32_t class_val;     /* rule.val, written to the class raster    */
  int32_t _pad;
} lt_rule;

/* settings.json semantics (README.md:46-85) minus target_date, which is folded into lt_scene. */
typedef struct {
  double line_cost;
  int32_t n_rules;
  int32_t pre_threshold_mode; /* LT_PRE_* */
  lt_rule rules[LT_MAX_RULES];
} lt_params;

/* Observation metadata shared by every pixel of a tile (all pixels of a co-registered stack see
 * the same acquisition dates). Built on the host from the dates and target_date
 * (land_trendr_amd/scene.py restates pick_winners' grouping, utils.py:503-517). */
typedef struct {
  int32_t n_obs;              /* K                                                          */
  int32_t n_years;            /* Y distinct calendar years, ascending                       */
  const int32_t* year;        /* [Y]   calendar year of slot y                              */
  const int32_t* slot_begin;  /* [Y+1] slot y covers order[slot_begin[y] .. slot_begin[y+1]) */
  const int32_t* order;       /* [K]   obs ids grouped by slot, caller's input order inside  */
  const int32_t* dist;        /* [K]   abs((target(year) - date).days) for order[k]          */
  const uint8_t* feb29_bad;   /* [Y]   1: target is Feb-29 and year y is not a leap year     */
} lt_scene;

/* Element types of raster planes (the GDAL band types a LandTrendr stack meets). */
enum { LT_T_F64 = 0, LT_T_I16 = 1, LT_T_U16 = 2, LT_T_I32 = 3, LT_T_F32 = 4, LT_T_U8 = 5,
       LT_T_U32 = 6, LT_T_I8 = 7, LT_T_I64 = 8,
       LT_T_BOOL = 9 };     /* a mask program's comparison / boolean nodes; never a raster type  */
/* An index_eqn program that is an integer linear form (lt_index_linearize): every arithmetic
 * node has the one integer type wrap_type, multiplications have a constant side, no division.
 * Its value for bands b[0..n_bands) is store_out(wrap(c0 + sum coef[s] * b[s])), the sum taken
 * modulo 2^64 (exact modulo 2^bits(wrap_type), as numpy's wrapping node by node), store_out the
 * load stage's store into out_type (lt_index.h). The analyze kernel evaluates it on the winning
 * observations' band values, so the index raster is never written (lt_tile_in.obs_bands). */
#define LT_LIN_MAX_BANDS 4
typedef struct {
  int32_t n_bands;            /* band planes the form reads (<= LT_LIN_MAX_BANDS)            */
  int32_t band_type;          /* LT_T_* of the band planes (I16 / U16 / U8 / I32)            */
  int32_t wrap_type;          /* LT_T_* of every arithmetic node                             */
  int32_t out_type;           /* LT_T_* of the index raster the form stands for              */
  int64_t c0;                 /* constant term, modulo 2^64                                  */
  int64_t coef[LT_LIN_MAX_BANDS]; /* coefficient of band plane s, modulo 2^64                */
} lt_index_lin;

typedef struct lt_index lt_index;  /* a compiled index_eqn program (lt_index_compile) */

typedef struct {
  int64_t n_pix;              /* P                                                          */
  int64_t stride;             /* elements between obs planes (>= n_pix)                     */
  const double* obs_val;      /* [K][stride] observation values (float(val), utils.py:357)  */
  const uint8_t* obs_valid;   /* [K][stride] 0 = cloud-masked (utils.py:353); NULL = all    */
  const void* obs_index;      /* [K][stride] the index raster in its stored type (typically */
                              /* what lt_index_apply wrote); used instead of obs_val if set */
  int32_t index_type;         /* LT_T_* of obs_index                                       */
  int32_t _pad;
  /* fused load stage: when obs_bands is set, obs_val / obs_index are ignored and the value of
   * obs o at pixel p is lin evaluated on band s = obs_bands[o*band_obs_stride + s*band_stride +
   * p*band_pix_stride] (rast_algebra + its store, utils.py:447-484, per winner). Planar bands
   * (lt_index_io's layout): band_pix_stride 1, band_stride >= n_pix. Pixel-interleaved bands
   * (one pixel's n_bands values side by side): band_stride 1, band_pix_stride = n_bands — the
   * two int16 bands of 'B1 - B2' are then one 32-bit load per winner */
  const void* obs_bands;
  int64_t band_obs_stride;    /* elements between the bands of consecutive obs              */
  int64_t band_stride;        /* elements between bands of one obs at one pixel             */
  int64_t band_pix_stride;    /* elements between consecutive pixels of one band            */
  lt_index_lin lin;
  /* the cloud mask as bit planes: bit (o % 32) of obs_valid_bits[(o / 32)*stride + p] is 1 when
   * obs o is valid at pixel p (utils.py:353); used instead of obs_valid when set. The winner pick
   * then reads ceil(K/32) words per pixel instead of one byte per observation */
  const uint32_t* obs_valid_bits;
  /* fused load stage for ANY index_eqn program (ABI 6): with obs_bands set and index a program
   * from lt_index_compile, the value of obs o at pixel p is that program evaluated on the bands
   * above and stored into its out_type, as lt_index_apply writes it; lin is ignored. The analyze
   * and resolve kernels are then JIT-compiled (hiprtc) with the program inlined into the winner
   * pick, once per program and kernel instance (cached in the context and on disk, lt_jit.h). The
   * band planes have the program's band_type and n_bands; any band type, planar or interleaved */
  const lt_index* index;
} lt_tile_in;

/* ---- load stage: settings.json index_eqn (utils.py:447-484 rast_algebra) -------------------- */
#define LT_MAX_PROG 64
#define LT_MAX_BANDS 16
enum { LT_OP_BAND = 1,      /* push band plane ival (0-based slot), in band_type               */
       LT_OP_CONST_I = 2,   /* push the integer ival                                            */
       LT_OP_CONST_F = 3,   /* push the double fval                                             */
       LT_OP_ADD = 4, LT_OP_SUB = 5, LT_OP_MUL = 6,
       LT_OP_DIV = 7,       /* Python 2 '/': floor division on integer types, true on floats    */
       LT_OP_FLOORDIV = 8,  /* '//'                                                             */
       LT_OP_NEG = 9,
       /* mask programs only (settings.json mask_eqn, lt_mask_*): rejected in an index program */
       LT_OP_EQ = 10, LT_OP_NE = 11, LT_OP_LT = 12, LT_OP_LE = 13, LT_OP_GT = 14, LT_OP_GE = 15,
                            /* compare: both operands cast to `type`, push a LT_T_BOOL; `type`  */
                            /* LT_T_BOOL (EQ / NE only) compares two booleans                    */
       LT_OP_AND = 16, LT_OP_OR = 17, LT_OP_XOR = 18, /* bitwise in an integer `type`, or of two */
                            /* booleans (`type` LT_T_BOOL)                                       */
       LT_OP_NOT = 19,      /* '~': bitwise in an integer `type`, logical on a boolean           */
       LT_OP_SHL = 20, LT_OP_SHR = 21 }; /* shift the top of stack by the literal ival, which is */
                            /* in [0, bits(type) - 1]; SHL wraps, SHR is arithmetic if signed    */
/* One postfix operation. `type` is the numpy result type of the node (binary ops: both operands
 * are cast to it first, as numpy does); integer results wrap. */
typedef struct {
  int32_t op;
  int32_t type;               /* LT_T_*                                                     */
  int64_t ival;
  double fval;
} lt_index_op;
/* A typed program built and validated by the host (land_trendr_amd/index_eqn.py). */
typedef struct {
  int32_t n_ops;
  int32_t n_bands;            /* band planes per observation                                */
  int32_t band_type;          /* LT_T_* of every band plane                                 */
  int32_t out_type;           /* LT_T_* the index raster is stored in (the template's type) */
  lt_index_op ops[LT_MAX_PROG];
} lt_index_prog;
/* Device buffers of one lt_index_apply: band s of obs o, pixel p at
 * bands[o*obs_stride + s*band_stride + p*band_pix_stride]; index of obs o, pixel p at
 * out[o*out_stride + p]. Planar bands: band_pix_stride 1 (or 0), band_stride >= n_pix.
 * Pixel-interleaved bands (the layout lt_tile_in.obs_bands reads fastest): band_stride 1,
 * band_pix_stride = the program's n_bands. */
typedef struct {
  int64_t n_pix;
  int64_t n_obs;
  int64_t obs_stride;
  int64_t band_stride;
  int64_t out_stride;
  const void* bands;
  void* out;
  int64_t band_pix_stride;
} lt_index_io;

/* ---- mask stage: settings.json mask_eqn (rast_algebra's mask_eqn, utils.py:447-484) ---------- */
typedef struct lt_mask lt_mask;  /* a compiled mask_eqn program (lt_mask_compile) */
/* A mask program is an lt_index_prog whose root is a LT_T_BOOL (out_type is ignored); a
 * LT_OP_CONST_I of type LT_T_BOOL pushes the boolean ival != 0. n_bands counts the band planes of
 * the stack it runs on; only the planes it names are read.
 * Device buffers of one lt_mask_apply: band s of obs o, pixel p at bands[o*obs_stride +
 * s*band_stride + p*band_pix_stride] (any non-negative strides, band_pix_stride >= 1); the
 * validity byte of obs o, pixel p at valid[o*valid_stride + p], set to 0 where the program is
 * false and never from 0 to non-zero. dropped (optional): the number of bytes turned from
 * non-zero to 0 is added to *dropped. */
typedef struct {
  int64_t n_pix;
  int64_t n_obs;
  int64_t obs_stride;
  int64_t band_stride;
  int64_t band_pix_stride;
  const void* bands;
  uint8_t* valid;
  int64_t valid_stride;       /* bytes between the validity rows of consecutive obs (>= n_pix) */
  uint64_t* dropped;          /* device counter to add to, or NULL                             */
} lt_mask_io;

/* ---- settings.json compiled on the host (for non-Python hosts) -------------------------------- */
/* The Python exception the reference raises for a rejected settings.json (lt_settings_compile). */
enum { LT_EXC_NONE = 0, LT_EXC_VALUE = 1, LT_EXC_KEY = 2, LT_EXC_TYPE = 3, LT_EXC_ATTRIBUTE = 4,
       LT_EXC_ZERO_DIVISION = 5, LT_EXC_OTHER = 6 };
typedef struct {
  lt_params params;           /* line_cost + label_rules, validated as LabelRule does            */
  int32_t target_year;        /* target_date 'YYYY-MM-DD' (parse_date, utils.py:194-202)         */
  int32_t target_month;
  int32_t target_day;
  int32_t n_index_bands;      /* band numbers index_eqn reads, ascending (utils.py:219-225);    */
  int32_t index_bands[LT_MAX_BANDS]; /* band plane s of lt_index_io holds band index_bands[s]   */
  lt_index_prog index;        /* index_eqn as a typed program (n_ops = 0 if the key is absent)  */
} lt_settings;

typedef struct {
  int64_t stride;             /* elements between year / rule planes (>= n_pix)             */
  int32_t* status;            /* [P]    LT_ST_* bits                                        */
  int32_t* n_years;           /* [P]    T: years present for the pixel                      */
  int16_t* winner;            /* [Y][stride] winning obs id, -1 = year absent for the pixel */
  double* val_raw;            /* [Y][stride] TrendlinePoint fields (classes.py:67-116);     */
  double* val_fit;            /*             absent years are written NaN / 0               */
  double* fit_m;
  double* fit_b;
  double* right_m;
  double* right_b;
  uint8_t* spike;
  uint8_t* vertex;
  uint8_t* matched;           /* [R][stride] change_labeling (utils.py:795-820)             */
  int32_t* class_val;         /*             rule.val if matched else LT_NODATA             */
  int32_t* onset_year;        /*             LT_NODATA if unmatched                         */
  int32_t* duration;
  double* magnitude;          /*             LT_NODATA if unmatched                         */
  double* initial_val;
} lt_tile_out;

/* Input of the label stage alone: an already analysed trendline per pixel. */
typedef struct {
  int64_t n_pix;
  int64_t stride;             /* elements between year planes                               */
  int32_t n_years;            /* Y slots                                                    */
  const int32_t* year;        /* [Y] HOST array: calendar year of each slot                 */
  const double* val_fit;      /* [Y][stride] device                                         */
  const uint8_t* vertex;      /* [Y][stride] device                                         */
  const uint8_t* present;     /* [Y][stride] device, 0 = no point in this slot; NULL = all  */
} lt_label_in;

/* ---- output raster assembly (output_reducer -> data2raster, utils.py:414-440) ----------------- */
enum { LT_RASTER_REFERENCE = 0, /* the reference's file: holder cast, then GDT_Byte (App. B #5)   */
       LT_RASTER_TYPED = 1 };   /* the corrected file: each value in out_type, fill elsewhere      */
enum { LT_SEL_ALL = 0, LT_SEL_NONZERO = 1, LT_SEL_EQUALS = 2 };
/* One output key's raster from a plane in device memory. A grid point p contributes when the
 * selector holds (the reducer emitted the key for it: matched[r][p] != 0 for '<rule>_<field>',
 * winner[y][p] == obs id for 'trendline/<date>-<attr>'); raster pixel dest[p] then holds its value
 * (the reference's holder[y_off, x_off] = float(value)), every other pixel NODATA. */
typedef struct {
  int64_t n_pix;              /* grid points                                                 */
  const void* plane;          /* [n_pix] device values, or NULL: const_value for every point */
  int32_t plane_type;         /* LT_T_I32 / LT_T_F64 / LT_T_U8 / LT_T_I16                     */
  int32_t sel_kind;           /* LT_SEL_*                                                    */
  const void* sel;            /* [n_pix] device: uint8 (NONZERO) or int16 (EQUALS) plane      */
  int32_t sel_value;          /* EQUALS: the obs id                                          */
  int32_t holder_type;        /* REFERENCE: LT_T_* of the holder (template type promoted)    */
  double const_value;         /* plane == NULL: the value (class_val: rule.val)              */
  const int64_t* dest;        /* [n_pix] device raster offsets, all distinct; NULL: dest[p]=p */
  int64_t n_out;              /* raster pixels (rows * cols)                                 */
  int32_t mode;               /* LT_RASTER_*                                                 */
  int32_t out_type;           /* REFERENCE: LT_T_U8; TYPED: LT_T_I32 / LT_T_F64 / LT_T_U8     */
  double fill;                /* TYPED: value of the pixels no selected point reaches        */
  void* out;                  /* [n_out] device                                              */
} lt_raster_job;

typedef struct lt_ctx lt_ctx;

int lt_abi_version(void);

/* settings.json (README.md:46-85, read by get_settings utils.py:241 and analysis_reducer
 * mr_land_trendr_job.py:98-118) -> lt_settings, on the host, no context needed. Validates
 * label_rules exactly as LabelRule (classes.py:32-64) and parses target_date / index_eqn as the
 * Python host does (land_trendr_amd/classes.py, scene.py, index_eqn.py): band_type / out_type are
 * the LT_T_* of the analysis rasters and of the stored index (-1: band_type), raster_count the
 * rasters' band count (0: unchecked). On failure returns LT_ERR_ARG (LT_ERR_LIMIT: too many
 * rules), sets *exc_kind to the LT_EXC_* of the exception the reference raises and writes its
 * message into err (NUL-terminated, at most err_cap bytes). Replaces, for a native host, the
 * Python LabelRule / parse_date / index_eqn.IndexProgram steps. */
int lt_settings_compile(const char* settings_json, int32_t pre_threshold_mode, int32_t band_type,
                        int32_t out_type, int32_t raster_count, lt_settings* out,
                        int32_t* exc_kind, char* err, int64_t err_cap);
/* Bind a context to a HIP device. Not thread-safe: one context per thread / GPU. */
int lt_ctx_create(int device, lt_ctx** out);
int lt_ctx_destroy(lt_ctx* ctx);
const char* lt_last_error(const lt_ctx* ctx);

/* Full analyze + label of one tile, asynchronous on `stream` (a hipStream_t; NULL = default).
 * Kernels: (1) analyze — winner pick, despike, the lazy segmented-least-squares DP, fits and
 * labels for every pixel whose optimal path is decided without LAPACK emulation; (2) resolve —
 * the pixels (1) deferred, with the exact-OPT screened DP. Calls on one context are ordered by
 * the stream: do not use one context from two streams at once. */
int lt_analyze_tile(lt_ctx* ctx, const lt_scene* scene, const lt_params* params,
                    const lt_tile_in* in, const lt_tile_out* out, void* stream);

/* lt_analyze_tile over n_tiles tiles of one scene (the reducer loop over a batch of grid-point
 * tiles, mr_land_trendr_job.py:83-126). Tile t's resolve kernels run on the context's own side
 * stream beside tile t+1's analyze kernel; every output is complete in `stream` order once the
 * call's work is done (`stream` waits for the last resolve). Same results as n_tiles calls of
 * lt_analyze_tile. */
int lt_analyze_tiles(lt_ctx* ctx, const lt_scene* scene, const lt_params* params, int n_tiles,
                     const lt_tile_in* ins, const lt_tile_out* outs, void* stream);

/* lt_analyze_tiles where tile t's analyze kernel first waits on ready[t] (a recorded hipEvent_t,
 * or NULL = no wait; `ready` itself may be NULL). The load stage (parse_mapper's rast_algebra,
 * utils.py:447-484) of later tiles can then run on another stream beside this call's analyze
 * kernels instead of all of it ahead of the call. */
int lt_analyze_tiles_after(lt_ctx* ctx, const lt_scene* scene, const lt_params* params,
                           int n_tiles, const lt_tile_in* ins, const lt_tile_out* outs,
                           void* const* ready, void* stream);

/* lt_analyze_tiles_after that also records, for every tile t with done[t] != NULL, the caller's
 * hipEvent_t done[t] once every output of tile t is complete (`done` itself may be NULL), and
 * with join == 0 returns WITHOUT making `stream` wait for the tiles' last stages: the caller then
 * orders later work on the done events (ABI 7; a multi-GPU runner posts tile t's label send after
 * done[t], so tile t's resolve stage keeps running beside tile t+1's analyze kernel). */
int lt_analyze_tiles_ev(lt_ctx* ctx, const lt_scene* scene, const lt_params* params, int n_tiles,
                        const lt_tile_in* ins, const lt_tile_out* outs, void* const* ready,
                        void* const* done, int32_t join, void* stream);

/* change_labeling alone (utils.py:795-820) on trendlines already in device memory. Writes the
 * rule planes of `out` and out->status (only LT_ST_PRE_THRESHOLD_ATTR can be set). */
int lt_label_tile(lt_ctx* ctx, const lt_label_in* in, const lt_params* params,
                  const lt_tile_out* out, void* stream);

/* ---- fit to vertex (FTV; an added export of ABI 8) ------------------------------------------------
 * The spikes and vertices an analysis found on one index, applied to a second index: the standard
 * LandTrendr product "segment with NBR, read wetness fitted at the same vertices". Input: the
 * winner / spike / vertex planes as lt_analyze_* wrote them and the second index's value of every
 * observation (one of obs_val / obs_index). Every pointer is a DEVICE pointer. */
typedef struct {
  int64_t n_pix;
  int64_t stride;          /* elements between the year planes of winner / spike / vertex */
  const int16_t* winner;   /* [Y][stride] DEVICE, as lt_analyze_* wrote them */
  const uint8_t* spike;
  const uint8_t* vertex;
  int64_t obs_stride;      /* elements between observation planes of the values (>= n_pix) */
  const double* obs_val;   /* [K][obs_stride], or NULL */
  const void* obs_index;   /* [K][obs_stride] in index_type (what lt_index_apply wrote), or NULL */
  int32_t index_type;      /* LT_T_* */
  int32_t _pad;
} lt_ftv_in;
/* vertices2eqns (utils.py:646-669) and eqns2fitted_points (utils.py:682-722) per pixel, bit for
 * bit, on given planes (land_trendr_amd/csrc/lt_ftv.h; one wave per 64 pixels, the fits in
 * lockstep over the context's x-set table), asynchronous on `stream`:
 *   present slots: winner[y] >= 0 (T of them); x(y) = year[y] - year[first present slot];
 *   val_raw[y] = the value of obs winner[y] (spikes included), NaN for absent slots;
 *   T == 0 / T == 1: status LT_ST_EMPTY / LT_ST_SINGLE_YEAR, every fit field NaN;
 *   else the non-spike present points are the fitting series, its flagged points the vertices,
 *   segment q the emulated-dgelsd least squares over the points from vertex q to vertex q+1
 *   inclusive (the last vertex takes the last segment's), and val_fit / fit_m / fit_b / right_m /
 *   right_b follow as in lt_analyze_*; LT_ST_NUMERIC is set when a fit fails.
 * Writes out->val_raw, val_fit, fit_m, fit_b, right_m, right_b ([Y][out->stride]) and out->status,
 * each only if non-NULL; every other field of `out` is ignored. Of `scene` only n_obs, n_years and
 * year are read. Malformed planes (fewer than two vertices with T >= 2; a winner outside
 * [-1, n_obs), which counts as absent) set LT_ST_NUMERIC, leave the fit values unspecified and
 * never read or write out of bounds. LT_ERR_ARG, with nothing launched, for a null scene / in /
 * out, null flag planes with n_pix > 0 and n_years > 0, stride, obs_stride or out->stride below
 * n_pix, both or neither of obs_val / obs_index, and an index_type that is no raster type;
 * LT_ERR_LIMIT as lt_analyze_tile gives it for the scene; LT_OK at once for n_pix == 0. */
int lt_ftv_tile(lt_ctx* ctx, const lt_scene* scene, const lt_ftv_in* in, const lt_tile_out* out,
                void* stream);

/* ---- vertex table (an added export of ABI 8) ------------------------------------------------------
 * A trendline in the form LandTrendr results are consumed in: one row per vertex per pixel, its
 * year and its fitted value, compacted from the per-year planes. Every Disturbance of
 * Trendline.parse_disturbances (classes.py:156-176) follows from it on any host: segment j has
 * onset vertex_year[j], duration vertex_year[j+1] - vertex_year[j], initial value vertex_fit[j]
 * and magnitude vertex_fit[j] - vertex_fit[j+1], one IEEE subtraction of two stored values.
 * Every pointer but `year` is a DEVICE pointer. */
typedef struct {
  int64_t n_pix;
  int64_t stride;             /* elements between the year planes (>= n_pix)                 */
  int32_t n_years;            /* Y slots                                                     */
  const int32_t* year;        /* [Y] HOST array: calendar year of each slot                  */
  const double* val_fit;      /* [Y][stride]                                                 */
  const uint8_t* vertex;      /* [Y][stride]                                                 */
  const double* val_raw;      /* [Y][stride], or NULL (then no vertex_raw)                   */
  const uint8_t* present;     /* [Y][stride], 0 = no point in this slot (as lt_label_in), or */
  const int16_t* winner;      /* [Y][stride], a point iff >= 0 (as lt_analyze_* wrote it);   */
                              /* at most one of the two; neither: every slot holds a point   */
} lt_vertex_in;
typedef struct {
  int64_t stride;             /* elements between the vertex planes (>= n_pix)               */
  int32_t max_vertices;       /* V: vertex slots per pixel, 1 .. LT_MAX_YEARS                */
  int32_t* n_vertices;        /* [P]         the pixel's full vertex count (may exceed V)    */
  int32_t* vertex_year;       /* [V][stride] calendar year of vertex j                       */
  double* vertex_fit;         /* [V][stride] val_fit at vertex j, bit for bit                */
  double* vertex_raw;         /* [V][stride] val_raw at vertex j, bit for bit                */
} lt_vertex_out;
/* The vertices of every pixel, in year order (land_trendr_amd/csrc/lt_vertex.h; a lane is a
 * pixel), asynchronous on `stream`, as label_pixel walks them:
 *   the slots that hold a point are taken in year order; the first of them is vertex 0 whatever
 *   its flag says; every later one with vertex != 0 is the next vertex;
 *   n_vertices[p] = their count (0: no point at all, 1: a single point or no later flag);
 *   for j < min(n_vertices, V): vertex_year[j][p] = year of the slot, vertex_fit[j][p] /
 *   vertex_raw[j][p] = the bits of val_fit / val_raw there (NaN payloads and -0.0 included);
 *   for min(n_vertices, V) <= j < V: LT_NODATA in every plane (-99 / -99.0).
 * Writes each of the four outputs only if non-NULL, every element [j < V][p < n_pix] exactly
 * once, and nothing else: no padding of a padded stride, no row >= V. No status is read: which
 * pixels count is the caller's decision. LT_ERR_ARG, with nothing launched, for a null in / out,
 * a negative n_pix or n_years, null val_fit or vertex (or year) with n_pix > 0 and n_years > 0, a
 * stride below n_pix, both present and winner, vertex_raw without val_raw, and max_vertices
 * outside [1, LT_MAX_YEARS]; LT_ERR_LIMIT for n_years > LT_MAX_YEARS or n_pix > LT_MAX_TILE_PIX;
 * LT_OK at once for n_pix == 0. */
int lt_vertex_table(lt_ctx* ctx, const lt_vertex_in* in, const lt_vertex_out* out, void* stream);

/* ---- MMU sieve (an added export of ABI 8) -----------------------------------------------------------
 * The minimum mapping unit of a change map: one rule's label plane over a rows x cols raster
 * (P = rows * cols, row-major: pixel q is row q / cols, column q % cols) grouped into patches, and
 * the patches below min_pixels dropped. A patch is a maximal set of pixels with matched != 0 and
 * one key, connected by 4- or 8-neighbourhood in the raster (the end of one row and the start of
 * the next are no neighbours); with key NULL every matched pixel has the same key. Every pointer
 * is a DEVICE pointer. */
typedef struct {
  int64_t rows, cols;
  uint8_t* matched;           /* [P] read; written only with apply                           */
  const int32_t* key;         /* [P], or NULL: one key for all (never written)               */
  int32_t connectivity;       /* 4 or 8                                                      */
  int32_t min_pixels;         /* >= 1: patches of fewer pixels are dropped (with apply)      */
  int32_t apply;              /* != 0: matched[q] = 0 wherever 0 < size[q] < min_pixels      */
  int32_t phases;             /* 0: all four launches. Else bit k (1, 2, 4, 8) runs launch  */
                              /* k + 1 alone, for timing tools: the outputs are complete     */
                              /* only after all four ran in order on the same buffers        */
} lt_sieve_in;
typedef struct {
  int32_t* root;              /* [P] smallest raster index of the pixel's patch; -1 where    */
                              /*     matched == 0                                            */
  int32_t* size;              /* [P] pixel count of the pixel's patch; 0 where unmatched     */
  void* workspace;            /* lt_sieve_workspace_bytes(rows, cols) bytes, 4-byte aligned; */
  int64_t workspace_bytes;    /* its contents before and after the call mean nothing         */
} lt_sieve_out;
/* Bytes of workspace lt_sieve_labels needs for a rows x cols raster (8 per pixel: a parent word
 * and a per-root counter; at least 8), or -1 for a negative size. Host only. */
int64_t lt_sieve_workspace_bytes(int64_t rows, int64_t cols);
/* Connected-component labelling by union-find (land_trendr_amd/csrc/lt_sieve.h, lt_sieve.hip):
 * four launches on `stream`, nothing read back, no workgroup waiting for another. root, size and
 * the applied matched are functions of the input alone (two calls agree in every element). Writes
 * root[q] and size[q] for every q < P, matched only with apply, key never, and nothing past P.
 * LT_OK at once for rows * cols == 0. LT_ERR_ARG, with nothing launched, for a null in / out /
 * matched / root / size / workspace, negative rows or cols, a connectivity other than 4 or 8,
 * min_pixels < 1, phases outside [0, 15], or workspace_bytes below lt_sieve_workspace_bytes(rows, cols); LT_ERR_LIMIT for
 * rows * cols > LT_MAX_TILE_PIX. */
int lt_sieve_labels(lt_ctx* ctx, const lt_sieve_in* in, const lt_sieve_out* out, void* stream);

/* ---- change maps (an added export of ABI 8) ---------------------------------------------------------
 * The map LandTrendr users publish: per pixel the one segment that is a loss (or a gain), passes
 * the filters and wins the sort, with its attributes; several maps from one pass over the planes.
 * A pixel's segments are those of label_pixel / Trendline.parse_disturbances (as lt_vertex_table
 * walks the vertices). A segment with left vertex (yl, fl) and right vertex (yr, fr), f the stored
 * val_fit:  onset_year = yl, duration = yr - yl, preval = fl, d = fl - fr (one IEEE subtraction),
 * magnitude = fabs(d), rate = magnitude / (double)duration (one IEEE division).
 * Every pointer but `year` is a DEVICE pointer. */
#define LT_MAX_CHANGE_MAPS 8
enum { LT_CM_LOSS = 0, LT_CM_GAIN = 1 };
enum { LT_CS_GREATEST = 0, LT_CS_LEAST, LT_CS_NEWEST, LT_CS_OLDEST,
       LT_CS_LONGEST, LT_CS_SHORTEST, LT_CS_STEEPEST, LT_CS_GENTLEST };
typedef struct {
  int32_t delta;              /* LT_CM_LOSS / LT_CM_GAIN                                     */
  int32_t sort;               /* LT_CS_*                                                     */
  int32_t index_sign;         /* +1: a loss is a fall of the index (sd = d); -1: a rise      */
                              /* (sd = -d). Loss keeps sd > 0, gain sd < 0; d == 0, -0.0 or  */
                              /* NaN is neither                                              */
  int32_t year_set;           /* != 0: year_lo <= onset_year <= year_hi                      */
  int32_t year_lo, year_hi;
  int32_t mag_op, dur_op, pre_op; /* LT_Q_UNSET / GT / LT / GE / LE on magnitude,            */
  int32_t _pad;                   /* (double)duration and preval against the values below    */
  double mag_val, dur_val, pre_val;
} lt_change_rule;
typedef struct {
  int64_t n_pix;
  int64_t stride;             /* elements between the year planes (>= n_pix)                 */
  int32_t n_years;            /* Y slots                                                     */
  const int32_t* year;        /* [Y] HOST array: calendar year of each slot                  */
  const double* val_fit;      /* [Y][stride]                                                 */
  const uint8_t* vertex;      /* [Y][stride]                                                 */
  const double* val_raw;      /* [Y][stride], or NULL (then no rmse / n_fit / dsnr)          */
  const uint8_t* present;     /* [Y][stride], 0 = no point in this slot, or                  */
  const int16_t* winner;      /* [Y][stride], a point iff >= 0; at most one of the two;      */
                              /* neither: every slot holds a point                           */
  const uint8_t* spike;       /* [Y][stride], or NULL (then no rmse / n_fit / dsnr)          */
} lt_change_in;
typedef struct {
  int64_t stride;             /* elements between the map planes (>= n_pix)                  */
  uint8_t* matched;           /* [M][stride] 1 where a segment was kept, else 0              */
  int32_t* onset_year;        /* [M][stride] the winner's attributes; LT_NODATA (-99 /       */
  int32_t* duration;          /*             -99.0) where matched is 0                       */
  double* magnitude;
  double* preval;
  double* rate;
  double* dsnr;               /* [M][stride] magnitude / rmse (+inf for a zero rmse;         */
                              /*             LT_NODATA with n_fit == 0)                      */
  double* rmse;               /* [P] the pixel's fit noise; LT_NODATA with n_fit == 0        */
  int32_t* n_fit;             /* [P] the points it is taken over                             */
} lt_change_out;
/* n_maps change maps of every pixel in one pass over its years (land_trendr_amd/csrc/lt_change.h;
 * a lane is a pixel), asynchronous on `stream`. Per map, a segment is kept iff its direction is
 * the rule's and every filter that is set compares *true* (a NaN operand drops it); among the kept
 * segments in year order the first is the winner and a later one replaces it only on a strict
 * improvement of the sort's key (greatest / least: magnitude, newest / oldest: onset_year,
 * longest / shortest: duration, steepest / gentlest: rate), so the first of equals wins.
 * The fit noise: over the slots that hold a point and have spike == 0, in year order,
 * r = val_raw - val_fit, acc = acc + r * r (product rounded, then the sum; no fused multiply-add),
 * n_fit their count, rmse = sqrt(acc / (double)n_fit), correctly rounded.
 * Writes each output only if non-NULL, every element [m < n_maps][p < n_pix] (rmse / n_fit:
 * [p < n_pix]) exactly once and nothing else: no padding of a padded stride, no row >= n_maps. No
 * status is read. LT_ERR_ARG, with nothing launched, for a null in / rules / out, negative sizes,
 * n_maps outside [1, LT_MAX_CHANGE_MAPS], null val_fit / vertex / year with n_pix > 0 and
 * n_years > 0, a stride below n_pix, both present and winner, rmse / n_fit / dsnr without both
 * val_raw and spike, a delta, sort, op or index_sign outside its set, and year_set with
 * year_lo > year_hi; LT_ERR_LIMIT for n_years > LT_MAX_YEARS or n_pix > LT_MAX_TILE_PIX; LT_OK at
 * once for n_pix == 0. */
int lt_change_maps(lt_ctx* ctx, const lt_change_in* in, int n_maps, const lt_change_rule* rules,
                   const lt_change_out* out, void* stream);
/* A label plane counted per key (the per-year area table of a change map, or of a label rule):
 * counts[k] += the pixels with matched != 0 and key == key_lo + k for k < n_bins, and
 * counts[n_bins] += the matched pixels whose key is outside the range. `counts` (DEVICE,
 * n_bins + 1 words) is added to, so the caller zeroes it; integer sums, so the result is a
 * function of the input alone. Asynchronous on `stream`. LT_ERR_ARG, with nothing launched, for a
 * null matched / key / counts, a negative n_pix and n_bins outside [1, 256]; LT_ERR_LIMIT for
 * n_pix > LT_MAX_TILE_PIX; LT_OK at once for n_pix == 0. */
int lt_label_counts(lt_ctx* ctx, const uint8_t* matched, const int32_t* key, int64_t n_pix,
                    int32_t key_lo, int32_t n_bins, uint64_t* counts, void* stream);
/* A label plane summed per zone and key (area, mean duration and mean magnitude per zone and onset
 * year; land_trendr_amd/csrc/lt_zonal.h). All planes are DEVICE pointers with unit stride over
 * n_pix pixels: matched, zone (a dense zone index), key, duration (or NULL), value (or NULL).
 * `table` (DEVICE) is [n_zones + 1][n_bins + 1][4] 64-bit words and is added to, so the caller
 * zeroes it. For every pixel with matched != 0: the row is zone if 0 <= zone < n_zones, else
 * n_zones; the column is key - key_lo (in 64 bits) if it lies in [0, n_bins), else n_bins; word 0
 * += 1; word 1 += duration (sign-extended) with a duration plane; and with a value plane and
 * v = value[p] not NaN, word 2 += (int64) rint(clamp(v, -2^30, 2^30) * 16.0) (round half to even;
 * +-inf clamp; |addend| <= 2^34) and word 3 += 1, so a mean is word 2 / 16 / word 3. Every word is
 * a two's-complement sum made with unsigned 64-bit adds: the result is a function of the input
 * alone, and equal on every path. No word can wrap within one call on a zeroed table (n_pix <=
 * 2^28); a caller that accumulates several calls owns that bound. path: 0 chooses, 1 forces the
 * block-private LDS table (LT_ERR_ARG unless (n_zones + 1) * (n_bins + 1) <= 1024), 2 the
 * wave-combined global adds. Asynchronous on `stream`; reads nothing back. LT_ERR_ARG, with
 * nothing launched, for a null matched / zone / key / table, a negative n_pix, n_bins outside
 * [1, 256], n_zones outside [1, LT_MAX_ZONES] and a path outside [0, 2]; LT_ERR_LIMIT for
 * n_pix > LT_MAX_TILE_PIX; LT_OK at once for n_pix == 0, before any other argument is looked at
 * (as lt_label_counts: with no pixel, null pointers and sizes outside their ranges are not
 * errors; every check but the negative n_pix applies to n_pix > 0 only). */
int lt_zonal_stats(lt_ctx* ctx, const uint8_t* matched, const int32_t* zone, const int32_t* key,
                   const int32_t* duration, const double* value, int64_t n_pix, int32_t key_lo,
                   int32_t n_bins, int32_t n_zones, int32_t path, uint64_t* table, void* stream);

/* Output raster assembly: n_jobs rasters (lt_raster_job), asynchronous on `stream`: a fill of
 * every raster pixel with NODATA's converted value, then the selected grid points scattered in
 * (one pass when dest is NULL). Replaces data2raster's per-point loop (utils.py:429-438) and the
 * holder -> GDT_Byte conversion GDAL does in array2raster (utils.py:374-412). */
int lt_raster_assemble(lt_ctx* ctx, const lt_raster_job* jobs, int n_jobs, void* stream);
/* Which observations won some pixel's year (the acquisition dates that get trendline keys,
 * classes.py:100-116): bit o of bits[] (device, (n_obs + 31) / 32 words, zeroed by the call) is
 * set iff winner[y * stride + p] == o for some y < n_years, p < n_pix. Asynchronous on `stream`. */
int lt_winner_presence(lt_ctx* ctx, const int16_t* winner, int64_t stride, int32_t n_years,
                       int64_t n_pix, int32_t n_obs, uint32_t* bits, void* stream);

/* ---- ingest: TIFF strips decoded on the device (ABI 8) -------------------------------------------
 * One strip-organised TIFF image whose compressed strips are in device memory: the arguments of
 * lt_tiff_decode_strips (include/lt_io.h), every pointer a DEVICE pointer. */
typedef struct {
  const uint8_t* file;      /* DEVICE: the bytes that hold every strip (the file, or a slice of it) */
  int64_t file_size;
  const uint64_t* offsets;  /* DEVICE [n_strips], relative to `file`                                */
  const uint64_t* counts;   /* DEVICE [n_strips]                                                    */
  int64_t n_strips;
  int32_t compression;      /* 1 or 5                                                               */
  int32_t predictor;        /* 1 or 2                                                               */
  int32_t bps;              /* bytes per sample: 1, 2, 4, 8                                         */
  int32_t big_endian;
  int64_t width, height;
  int32_t bands, planar;    /* planar 1 (chunky: de-interleaved here) or 2                          */
  int64_t rows_per_strip;
  void* out;                /* DEVICE [bands][height][width], native byte order                     */
  int32_t* err;             /* DEVICE one word: zeroed by the call, then the LT_IO_ERR_* of some
                               failing strip (first writer wins, atomicCAS from 0), else 0          */
} lt_strips_job;
/* lt_tiff_decode_strips (lt_io.h) for n_jobs images whose compressed strips are in device memory,
 * asynchronous on `stream`; same results, same zero padding of short strips, same ignored extra
 * strips. LT_ERR_ARG for what the host function rejects (any compression but 1 and 5 among it:
 * Deflate is lt_tiff_decode_chunks_dev's) and for strips of 1 MiB or more decoded.
 * Each job is decoded as the lt_chunks_job (below) with tiled 0, chunk_w = width, chunk_h =
 * rows_per_strip and n_chunks = n_strips, by lt_tiff_decode_chunks_dev's kernel and out of the same
 * context scratch, with at most 256 MiB of chunk buffers (chunky strips) in flight. A failing
 * strip's rows are unspecified; every other strip is decoded. */
int lt_tiff_decode_strips_dev(lt_ctx* ctx, const lt_strips_job* jobs, int n_jobs, void* stream);

/* ---- ingest: TIFF tiles and Deflate decoded on the device (an added export of ABI 8) -------------
 * One TIFF image, strip- or tile-organised, whose compressed chunks (strips or tiles) are in
 * device memory: the arguments of lt_tiff_decode_chunks (include/lt_io.h), every pointer a DEVICE
 * pointer. lt_strips_job's fields with n_chunks for n_strips and chunk_h for rows_per_strip, plus
 * chunk_w and tiled. */
typedef struct {
  const uint8_t* file;      /* DEVICE: the bytes that hold every chunk (the file, or a slice of it) */
  int64_t file_size;
  const uint64_t* offsets;  /* DEVICE [n_chunks], relative to `file`                                */
  const uint64_t* counts;   /* DEVICE [n_chunks]                                                    */
  int64_t n_chunks;         /* at least the image's: ceil(H / chunk_h) strips, or
                               ceil(W / chunk_w) * ceil(H / chunk_h) tiles, per band when planar 2  */
  int32_t compression;      /* 1, 5 or 8 (Deflate; the caller maps 32946 to 8)                      */
  int32_t predictor;        /* 1 or 2                                                               */
  int32_t bps;              /* bytes per sample: 1, 2, 4, 8                                         */
  int32_t big_endian;
  int64_t width, height;
  int32_t bands, planar;    /* planar 1 (chunky: de-interleaved here) or 2                          */
  int64_t chunk_w, chunk_h; /* tiles: the tile's size (tags 322, 323); strips: the image's width
                               and the rows per strip                                               */
  int32_t tiled;            /* 0 strips (the last one short), 1 tiles (all full, edges clipped)     */
  void* out;                /* DEVICE [bands][height][width], native byte order                     */
  int32_t* err;             /* DEVICE one word: zeroed by the call, then the LT_IO_ERR_* of some
                               failing chunk (first writer wins, atomicCAS from 0), else 0          */
} lt_chunks_job;
/* lt_tiff_decode_chunks (lt_io.h) for n_jobs images whose compressed chunks are in device memory,
 * asynchronous on `stream`; same results, same zero padding of short chunks, same ignored extra
 * chunks. LT_ERR_ARG, before anything is launched, for a null pointer, a non-positive size, a
 * compression, predictor or planar value outside the lists above, strips whose chunk_w is not the
 * width, fewer chunks than the image has, and chunks of 1 MiB or more decoded. One lane per chunk
 * (land_trendr_amd/csrc/lt_chunk.h over lt_lzw_core.h and lt_inflate_core.h, the sources
 * liblt_io.so's lt_tiff_decode_chunks is compiled from), at most 32768 in flight, 16 images to a
 * launch; a launch with a compression 8 image runs the kernel compiled with Deflate (a wave's
 * Huffman tables in LDS), any other the one without. The context owns the LZW string tables (16 KB
 * a lane, LZW images only) and the lanes' chunk buffers (tiles and chunky chunks; at most 1 GiB),
 * grown on demand, one set per stream, shared with lt_tiff_decode_strips_dev. A failing chunk's
 * pixels are unspecified; every other chunk is decoded. */
int lt_tiff_decode_chunks_dev(lt_ctx* ctx, const lt_chunks_job* jobs, int n_jobs, void* stream);

/* ---- output: TIFF strips encoded on the device (an added export of ABI 8) -------------------------
 * One raster in device memory to its strips: the arguments of lt_tiff_encode_strips
 * (include/lt_io.h), every pointer a DEVICE pointer. */
typedef struct {
  const void* in;          /* DEVICE [bands][rows][cols], little-endian samples; never written     */
  int32_t bands;
  int32_t bps;             /* bytes per sample: 1, 2, 4, 8                                          */
  int64_t rows, cols, rows_per_strip;
  int32_t compression;     /* 1 or 5                                                                */
  int32_t predictor;       /* 1 or 2 (horizontal differencing, integer wrap)                        */
  uint8_t* out;            /* DEVICE [cap]: the strips back to back, band-major then row order      */
  int64_t cap;
  int64_t* strip_sizes;    /* DEVICE [ceil(rows / rows_per_strip) * bands]                          */
  int64_t* total;          /* DEVICE one word: the bytes in `out`, or a negative LT_IO_ERR_*
                              (LT_IO_ERR_SPACE when cap is too small: the strips that fit whole
                              below cap are in place, nothing is written at or past out + cap)      */
} lt_encode_job;
/* lt_tiff_encode_strips (lt_io.h) for n_jobs rasters in device memory, asynchronous on `stream`:
 * the same bytes, sizes and total. LT_ERR_ARG for what the host function rejects and for strips of
 * 1 MiB or more of raw bytes. One lane per strip (the LZW core of land_trendr_amd/csrc/
 * lt_lzw_core.h, the source liblt_io.so's lt_lzw_encode_core is compiled from), at most 32768 in
 * flight; the context owns the lanes' dictionaries (32 KB a lane) and the slots they encode into
 * (at most 1 GiB each, grown on demand); a scan and a packing kernel lay the strips out.
 * Compression 1 is one coalesced kernel straight into `out`. */
int lt_tiff_encode_strips_dev(lt_ctx* ctx, const lt_encode_job* jobs, int n_jobs, void* stream);

/* ---- ingest: rasters sampled at the grid points on the device (an added export of ABI 8) ---------
 * The reference samples every raster and every cloud mask at the template's grid points
 * (pt2val, utils.py:285-297; apply_grid, utils.py:328-359). In the job's raster
 * order grid pixel p = r * grid_w + c has the coordinates (x of column c, y of row r), so the
 * source column depends on c alone and the source row on r alone: the caller computes the two
 * offset axes on the host (ingest.axis_offsets: numpy's negative-index wrap applied, -1 where
 * pt2val raises) and the device does the integer gather. */
enum { LT_SAMPLE_BANDS = 0, LT_SAMPLE_MASK = 1 };
typedef struct {
  const void* src;            /* DEVICE [src_bands][src_h][src_w], native byte order        */
  int32_t bps, src_bands;     /* bytes per sample: 1, 2, 4, 8                               */
  int64_t src_h, src_w;
  const int32_t* xoff;        /* DEVICE [grid_w]: source column of grid column c, -1 = off  */
  const int32_t* yoff;        /* DEVICE [grid_h]: source row of grid row r, -1 = off        */
  int64_t grid_w, grid_h;
  int64_t p0, n;              /* grid pixels p0 .. p0+n-1, p = r * grid_w + c               */
  int32_t n_sel, sel[16];     /* source band of output plane b (MASK: sel[0] only)          */
  void* out; int64_t out_stride; /* plane b at out + b*out_stride samples; pixel p0+i at i  */
  uint8_t* valid;             /* DEVICE [n]                                                 */
  int32_t mode;
} lt_sample_job;
/* n_jobs sampling jobs, in order and asynchronous on `stream`. With on = xoff[c] >= 0 &&
 * yoff[r] >= 0 for pixel i of a job:
 *   LT_SAMPLE_BANDS  out[b][i] = on ? src[sel[b]][yoff[r] * src_w + xoff[c]] : 0 (a 64-bit index),
 *                    valid[i] = on: what np.take at grid_offsets' indices, zero where pt2val
 *                    raises, gives per band (ingest.ingest_stack);
 *   LT_SAMPLE_MASK   valid[i] &= !(on && every byte of the sample of band sel[0] is zero): a grid
 *                    point whose mask value is 0 is skipped (utils.py:351-356); `out` is unused.
 * LT_ERR_ARG, with nothing launched, for a bps other than 1, 2, 4, 8, a bad mode, n_sel outside
 * 1..16, a sel outside the source's bands, a negative size (out_stride < n in BANDS mode), sizes of
 * 2^31 or more, p0 + n > grid_w * grid_h, a null pointer of a job with n > 0, and src or out not
 * aligned to bps. Offsets at or past src_w / src_h are the caller's to exclude; the kernel treats
 * them as off the raster and never reads outside `src`. The per-pixel logic is
 * land_trendr_amd/csrc/lt_sample.h, the source liblt_io.so's lt_grid_sample is compiled from. */
int lt_grid_sample_dev(lt_ctx* ctx, const lt_sample_job* jobs, int n_jobs, void* stream);

/* Stage timing: when enabled, each lt_analyze_tile brackets its kernels with hipEvents on the
 * launch stream; lt_ctx_stage_ms returns the accumulated milliseconds per stage
 * (0 = analyze: every pixel with the lazy DP, 1 = resolve: the deferred pixels with the exact-OPT
 * DP) since the last call, and the number of lt_analyze_tile calls. */
int lt_ctx_set_timing(lt_ctx* ctx, int enable);
int lt_ctx_stage_ms(lt_ctx* ctx, double* ms_out, int n_stages, int64_t* n_launches);
/* Pixels the last lt_analyze_tile deferred to the resolve stage (synchronous read). */
int lt_ctx_last_deferred(lt_ctx* ctx, int64_t* n_deferred);

/* Load stage. lt_index_codegen writes the HIP source generated for `prog` (for inspection and the
 * CPU tests; returns the length, or a negative LT_ERR_*). lt_index_compile builds it with hiprtc
 * for the context's device (cached per program inside the context; LT_ERR_JIT with the compiler
 * log in lt_last_error on failure). lt_index_apply computes the index raster of every observation
 * of a tile — rast_algebra's eval, then the store into out_type — asynchronously on `stream`. */
int lt_index_codegen(const lt_index_prog* prog, char* buf, int64_t cap);
int lt_index_compile(lt_ctx* ctx, const lt_index_prog* prog, lt_index** out);
int lt_index_apply(lt_ctx* ctx, const lt_index* fn, const lt_index_io* io, void* stream);
/* The linear form of `prog` (see lt_index_lin) for the analyze kernel's fused load stage, or
 * LT_ERR_ARG when the program is not one (a division, a float node, a product of two band
 * terms, mixed integer node types, a band type the kernel does not read, more than
 * LT_LIN_MAX_BANDS bands): such programs keep lt_index_apply. Host only, no context. */
int lt_index_linearize(const lt_index_prog* prog, lt_index_lin* out);

/* Mask stage (settings.json mask_eqn). lt_mask_codegen writes the HIP source generated for the
 * mask program `prog` (host only; the length, or a negative LT_ERR_*). lt_mask_compile builds it
 * with hiprtc for the context's device (cached per program inside the context, the handle freed
 * with the context; LT_ERR_JIT with the compiler log in lt_last_error on failure). lt_mask_apply
 * clears the validity bytes of the observations the program is false on, asynchronously on
 * `stream`; LT_ERR_ARG (nothing launched) for null or negative arguments. The C settings compiler
 * (lt_settings_compile) does not read mask_eqn: a non-Python host builds the program itself. */
int lt_mask_codegen(const lt_index_prog* prog, char* buf, int64_t cap);
int lt_mask_compile(lt_ctx* ctx, const lt_index_prog* prog, lt_mask** out);
int lt_mask_apply(lt_ctx* ctx, const lt_mask* fn, const lt_mask_io* io, void* stream);

/* ---- JIT kernels (lt_tile_in.index; ABI 7) -------------------------------------------------------
 * A tile carrying an index_eqn program runs analyze / resolve kernels compiled for it (hiprtc,
 * lt_jit.h) from kernel headers embedded in this library. Until a tile's module is ready, or if its
 * compile fails, the tile runs on the precompiled kernels instead — a linear program through its
 * lt_index_lin form, any other through its index raster (the program's load kernel into a context
 * scratch buffer) — with the same results; lt_ctx_jit_stats counts both kinds of tile. */
enum { LT_JIT_SYNC = 0,    /* a launch needing a module compiles it first (the default)        */
       LT_JIT_ASYNC = 1 }; /* modules compile on worker threads; tiles launched before theirs
                              is ready take the precompiled kernels                             */
int lt_ctx_set_jit_mode(lt_ctx* ctx, int32_t mode);
/* Compile (wait != 0) or start compiling (wait == 0, on a worker thread) the module a
 * lt_analyze_tiles call with this scene, params, tile and output set would use, so that no launch
 * waits for hiprtc (e.g. every scene of a mosaic before the first tile). LT_OK also when `in`
 * carries no program; LT_ERR_JIT (the log in lt_last_error) when a waited-for compile failed. */
int lt_jit_prepare(lt_ctx* ctx, const lt_scene* scene, const lt_params* params,
                   const lt_tile_in* in, const lt_tile_out* out, int32_t wait);
typedef struct {
  int64_t jit_tiles;       /* tiles launched on JIT kernels                                    */
  int64_t fallback_tiles;  /* tiles with a program launched on the precompiled kernels         */
  int64_t compiles;        /* modules compiled with hiprtc                                     */
  int64_t disk_hits;       /* modules read from the disk cache (LT_JIT_CACHE)                  */
  int64_t failures;        /* modules whose compile or load failed                             */
  int64_t modules;         /* modules loaded now (least recently used unloaded past a cap)     */
  int64_t evictions;       /* modules unloaded                                                 */
  int64_t pending;         /* compiles still running                                           */
} lt_jit_stats;
/* The context's JIT counters since creation and the last JIT failure message (NUL-terminated into
 * last_error, at most cap bytes; may be NULL). Loads modules whose compile has finished. */
int lt_ctx_jit_stats(lt_ctx* ctx, lt_jit_stats* out, char* last_error, int64_t cap);
/* The module source the context would compile for a tile of this scene and params carrying
 * `prog` (masked: the tile has a cloud mask; year_out: a per-year plane is requested), with the
 * launch constants (LT_JIT_SRC_SPEC) and the scene's tables (LT_JIT_SRC_SCENE); host only, for
 * inspection and ahead-of-time builds. Returns the length, or a negative LT_ERR_*. */
enum { LT_JIT_SRC_SPEC = 1, LT_JIT_SRC_SCENE = 2, LT_JIT_SRC_FIELDS = 4 };
/* LT_JIT_SRC_FIELDS: flags bits 8.. carry the launch's non-null output planes as the kernels'
 * LT_FIELD_* bits (status 0, n_years 1, matched 2, class_val 3, onset_year 4, duration 5,
 * magnitude 6, initial_val 7, winner 8, val_raw 9, val_fit 10, fit_m 11, fit_b 12, right_m 13,
 * right_b 14, spike 15, vertex 16), as the context specialises a launch for them. */
int lt_jit_source(const lt_scene* scene, const lt_params* params, const lt_index_prog* prog,
                  int32_t masked, int32_t year_out, int32_t flags, char* buf, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif
