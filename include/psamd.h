/*
 * psamd.h -- C ABI of the MI355X-native particle-system step ("psamd").
 *
 * Drop-in boundary for the per-step hot path of abraj/particleSystem: the three
 * stage bodies the reference registers with pmlib (task 3 init_iframe, task 8
 * build_grid, task 6 calc_forces; DoParallelProcess loop, particleSystem.cpp
 * 1843-1928) plus the one-off setup stages that create their inputs.  Plain
 * pointers and sizes only; every function returns a psamd_status and never
 * exits or throws across the boundary (the reference printf+exit(1)s instead,
 * particleSystem.cpp:937-938, app.cu:429-431).
 *
 * Citations: "ps.cpp" = source/code/src/particleSystem.cpp, "psCUDA.cu" =
 * source/code/src/particleSystemCUDA.cu, the rest under source/code/inc/.
 *
 * Ownership: the library owns all device memory and its HIP streams.  Host
 * buffers passed in or out belong to the caller and are only touched during
 * the call.  One context is used by one host thread at a time (the reference's
 * driver thread blocks in pmWaitForTaskCompletion the same way, ps.cpp:1716).
 */
#ifndef PSAMD_H
#define PSAMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSAMD_ABI_VERSION 8

#define PSAMD_MAX_RANKS 64

typedef enum psamd_status {
    PSAMD_OK = 0,
    PSAMD_ERR_INVALID_ARG   = 1,  /* null pointer, out-of-range index, bad config          */
    PSAMD_ERR_NO_DEVICE     = 2,  /* no usable HIP device: the product has no CPU fallback */
    PSAMD_ERR_HIP           = 3,  /* a HIP runtime call failed (see psamd_last_error)      */
    PSAMD_ERR_OUT_OF_MEMORY = 4,
    PSAMD_ERR_OUTSIDE_BOX   = 5,  /* fill: "Particle location OUTSIDE box", ps.cpp:954-957 */
    PSAMD_ERR_QUEUE_EMPTY   = 6,  /* fill: "Overflow (Reserved space full)", ps.cpp:936-939*/
    PSAMD_ERR_CELL_OVERFLOW = 7,  /* a cell holds more than MAX_PARTICLES_PER_CELL and the
                                     overflow policy is PSAMD_OVERFLOW_ERROR               */
    PSAMD_ERR_STATE         = 8,  /* stage called out of order (e.g. calc before build)    */
    PSAMD_ERR_UNSUPPORTED   = 9
} psamd_status;

/* config.flags */
#define PSAMD_FLAG_EXPLOSIONS   0x1u  /* births enabled (ps.cpp:1306-1333) with the counter-based RNG below */
#define PSAMD_FLAG_FAST_MATH    0x2u  /* FMA/rsq pair arithmetic: NOT bit-identical to the reference, see DESIGN.md.  Only the pair
                                         sums differ (everything after them is the exact path's); every pair is formed by the same
                                         operations in the same order whatever the launch shape, so the mode gives the same bytes
                                         from run to run, with graphs on or off, and as the union of slabs */
#define PSAMD_FLAG_ALL_PAIRS    0x4u  /* force walk over EVERY cell, not only the 27-cell stencil (the reference has only the
                                         cutoff, app.cu:352-452): the stencil first, in the reference's order, then the other
                                         cells in index order -- so a cloud that fits a 2x2x2 block of cells gets the cutoff
                                         result bit for bit.  Collisions stay short-range.  With world > 1 every rank
                                         contributes the snapshot of its own cells to an all-gather once per step
                                         (allg_out -> allg_in below) and walks the gathered buffer in the same order. */
#define PSAMD_FLAG_EULER        0x8u  /* position update x += v*dt (explicit Euler) instead of the reference's
                                         x += v*dt + 0.5*a*dt*dt (ps.cpp:1274-1276); the velocity update is the same.
                                         dx is the fp32 product v*dt alone; the MAX_DX clamp, the wrap and the segment
                                         change act on it as they do on the reference's dx */
#define PSAMD_FLAG_FAR_MONOPOLE 0x10u /* long-range gravity at a small multiple of the cutoff step's cost: the stencil first, in the
                                         reference's order, then every OTHER cell of the box as one body -- its total mass at its
                                         centre of mass.  See "long-range gravity" below.  Collisions stay short-range.  Not with
                                         PSAMD_FLAG_ALL_PAIRS (PSAMD_ERR_INVALID_ARG); world == 1 only, unless PSAMD_FLAG_FAR_SLAB is set */
#define PSAMD_FLAG_FAR_PYRAMID 0x20u  /* long-range gravity whose cost grows with log G instead of G^3: the stencil first, then coarser
                                         cells for farther mass -- a pyramid of monopoles.  See "a pyramid of monopoles" below.  Not
                                         with PSAMD_FLAG_ALL_PAIRS or PSAMD_FLAG_FAR_MONOPOLE (PSAMD_ERR_INVALID_ARG); world == 1 only,
                                         unless PSAMD_FLAG_FAR_SLAB is set */
#define PSAMD_FLAG_FAR_QUADRUPOLE 0x40u /* a modifier of PSAMD_FLAG_FAR_PYRAMID (alone: PSAMD_ERR_INVALID_ARG): every cell of the
                                         pyramid also carries its second moments, and every far body adds its quadrupole term.  See
                                         "quadrupoles on the pyramid" below */
#define PSAMD_FLAG_FAR_SLAB 0x80u     /* a modifier of PSAMD_FLAG_FAR_MONOPOLE and PSAMD_FLAG_FAR_PYRAMID (alone, or with
                                         PSAMD_FLAG_ALL_PAIRS: PSAMD_ERR_INVALID_ARG): the host says that it all-gathers allg_out
                                         into allg_in between slab_build and slab_pairs, so the far field is served with
                                         world > 1.  With world == 1 no message exists and every byte is what the context
                                         computes without the flag.  See "far field on slabs" below */

/* Runtime form of the reference's compile-time configuration, common.h:12-70.
 * psamd_default_config() fills in the shipped values. */
typedef struct psamd_config {
    int32_t  max_particles_num;  /* MAX_PARTICLES_NUM        common.h:12 */
    int32_t  x_factor;           /* X_FACTOR                 common.h:13 */
    int32_t  chunk_factor;       /* CHUNK_FACTOR             common.h:29 */
    int32_t  chunk_dim;          /* CHUNK_DIM                common.h:30 */
    double   cell_size;          /* CELL_SIZE                common.h:52 */
    double   eps2;               /* EPS2                     common.h:53 */
    double   collision_radius;   /* COLLISION_RADIUS         common.h:54 */
    double   particle_weight;    /* PARTICLE_WEIGHT_DEFAULT  common.h:55 */
    double   dt;                 /* DT                       common.h:69 */
    double   max_v;              /* MAX_V                    common.h:66 */
    double   explosion_speed;    /* EXPLOSION_SPEED          common.h:67 */
    double   life_steps;         /* the 300 in PARTICLE_LIFE common.h:58 */
    int32_t  device;             /* HIP device ordinal                    */
    uint32_t flags;              /* PSAMD_FLAG_*                          */
    uint64_t seed;               /* explosion RNG seed (RAND_SEED, common.h:56) */
    /* Multi-GPU: world > 1 makes this context ONE SLAB of the system (see "slab partition"
     * below): it holds only the segments of its cell layers -- their slots, particles and
     * free-slot queues -- and steps through the psamd_slab_* stage calls.  cuts[0..world]
     * (cell-layer boundaries along i3, cuts[0] = 0, cuts[world] = grid_dim, at least two
     * layers per rank) overrides the balanced partition when cuts[world] != 0. */
    int32_t  rank;
    int32_t  world;
    int32_t  halo_cap_cell;      /* bodies per cell, ON AVERAGE OVER A CELL LAYER, a halo message has room for (any one cell up to its list
                                    capacity: the room is pooled); 0 = MAX_PARTICLES_PER_CELL (never overflows) */
    int32_t  xfer_cap;           /* records a transfer message carries per step and direction (particles changing owner) TO BEGIN WITH;
                                    0 = a quarter of what a cell layer can hold.  The ranks raise it together when the traffic asks for
                                    it and lower it again, never below this number, when the traffic has gone (see xfer_cap_max) */
    int32_t  cuts[PSAMD_MAX_RANKS + 1];
    /* Not in the reference (BASELINE.json asks for them; nothing there can pin them): */
    double   drag;               /* linear drag k >= 0: the acceleration that is integrated and stored is a - k*v; 0 = the
                                    reference's arithmetic, untouched.  For every particle the step integrates, per axis and in
                                    fp32: a' = RN(a - RN(k*v)) with k = (float)drag -- two roundings, no fused multiply-add;
                                    a' enters the position and the velocity update alike and is what ax, ay, az keep.  Where k*v is
                                    not a number, a' is that not-a-number bit for bit (its sign is not left to the subtraction) */
    double   force_sign;         /* +1 gravity (reference), -1 repulsion: multiplies every mass in the force term; 0 reads as +1.
                                    The collision scan does not see it; w in the particle records and in the T_DATA rows stays
                                    unsigned (the sign lives in the pair stage's own snapshot, in the halo messages and in the
                                    all-gather block) */
    int32_t  xfer_cap_max;       /* how far the transfer messages may grow: their BUFFERS have this room from the start, the bytes that
                                    travel are xfer_cap's and follow the traffic.  Every rank reports in its status record how many records it
                                    sent in the step before; all ranks see all records and apply the same rule -- twice (the busiest rank's
                                    count + four times its rise since the step before), from the step after next; down to that number again
                                    when it is no more than half of what the messages hold -- so both
                                    ends of every message change size in the same step with no negotiation round (psamd_slab_buffers_get().xfer_bytes is the size to post,
                                    read it after psamd_slab_apply).  0 = what two cell layers and their children can hold (a step's
                                    worst case: the reference ships whole segments, ps.cpp:431-487); < xfer_cap: no growth. */
    int32_t  reserved0;
} psamd_config;

/* Sizes DoInit derives (ps.cpp:2204-2222), in elements. */
typedef struct psamd_sizes {
    int32_t grid_dim, num_cells, num_chunks, cells_per_chunk;
    int32_t max_per_cell, max_per_chunk;
    int32_t container_size;      /* nParticles = nTdata = nQueue        */
    int32_t queue_info_size;     /* nQueueInfo                           */
    int64_t n_chunkgrid;         /* NUM_CHUNKS*(1+MAX_PARTICLES_PER_CHUNK) */
    int64_t n_cellgrid;          /* NUM_CELLS*(1+MAX_PARTICLES_PER_CELL)   */
    int32_t n_pkgdistrib;        /* NUM_CHUNKS*27 PAIRs                  */
    int32_t seg_count[4], seg_size_t[4], seg_size[4]; /* types 1,2,4,8  */
} psamd_sizes;

/* Event counts of the last psamd_calc_forces / psamd_step call(s), cumulative. */
typedef struct psamd_counters {
    int64_t deaths_age, deaths_collision, survives, integrated;
    int64_t relocations, relocations_lost, births, births_failed, cell_overflow_kills;
    int64_t steps;
    int64_t particles_processed; /* sum over steps of the live particles at build_grid */
    int64_t max_ops_one_queue;   /* most free-slot-queue operations one segment got in one step */
} psamd_counters;

/* Raw device pointers of the SoA state, for plumbing (collectives, interop).
 * Valid until psamd_destroy.  Layouts are described in DESIGN.md section 3. */
typedef struct psamd_device_view {
    /* slot arrays hold the OWNED slots only, back to back (world == 1: the whole container) */
    void    *pos4;        /* float4[container]  x,y,z,w                         */
    void    *vel4;        /* float4[container]  vx,vy,vz,age                    */
    void    *acc4;        /* float4[container]  ax,ay,az,fertility_age          */
    void    *cell;        /* int[container]     cell index, -1 = free slot      */
    void    *pflags;      /* uint8[container]   bit0 = is_parent                */
    void    *sorted_id;   /* int[container]     slot ids, cell-major, id-ascending in a cell */
    void    *snap_soa;    /* float[4][sorted_cap] snapshot in sorted order: x, y, z, w_eff planes */
    void    *force4;      /* float4[sorted_cap] sorted order: force records of the lent region, hand-off scratch (the own cells'
                             records live by slot since ABI 6: read them with psamd_download_force4) */
    void    *cell_start;  /* int[num_cells+1]   exclusive prefix of cell counts */
    int64_t  container_size;
    int32_t  num_cells;
    int32_t  live;        /* live particles at the last build_grid             */
    int64_t  sorted_cap;  /* plane stride of snap_soa, in floats                */
    void    *stream;      /* hipStream_t the stages are enqueued on            */
} psamd_device_view;

/* Fields of psamd_export_live / psamd_download_live (the bits of `fields`) */
#define PSAMD_EXPORT_POS  0x1u   /* float4 x,y,z,w                 */
#define PSAMD_EXPORT_VEL  0x2u   /* float4 vx,vy,vz,age            */
#define PSAMD_EXPORT_ACC  0x4u   /* float4 ax,ay,az,fertility_age  */
#define PSAMD_EXPORT_ID   0x8u   /* int32 global slot id (P_DATA_TYPE.id) */
#define PSAMD_EXPORT_CELL 0x10u  /* int32 cell                     */
#define PSAMD_EXPORT_ALL  0x1fu

/* Statistics of the live particles.  Every term is formed in fp64 from the fp32 fields; a particle whose position or
 * velocity (x, y, z, vx, vy, vz) is not a finite number counts in `live` and `nonfinite` and nowhere else.  The sums
 * run in a fixed order (a fixed tree inside each tile of 4096 owned slots, then the tiles in index order), so they are
 * the same bits from run to run, with graphs on or off, for a given context geometry.  No live particle: the sums
 * are 0, lo / age_min are +inf and hi / age_max are -inf. */
typedef struct psamd_live_stats {
    int64_t live;
    int64_t nonfinite;
    double  mass;            /* sum w                                   */
    double  momentum[3];     /* sum w*v                                 */
    double  kinetic;         /* sum 0.5*w*|v|^2                         */
    double  mass_moment[3];  /* sum w*x: the centre of mass is mass_moment / mass */
    double  lo[3], hi[3];    /* bounding box of the positions           */
    double  age_min, age_max, age_sum;
} psamd_live_stats;

/* What psamd_export_live writes and where (device pointers).  A field whose bit is set needs its pointer (float4
 * arrays 16-byte aligned, int32 arrays 4-byte aligned, `capacity` entries each); the pointer of a field that is not
 * asked for is ignored.  count_dev / stats_dev: optional; NULL = not wanted. */
typedef struct psamd_export {
    uint32_t fields;          /* PSAMD_EXPORT_* bits                    */
    int32_t  reserved;        /* 0                                      */
    void    *pos4, *vel4, *acc4;
    void    *id, *cell;
    int64_t  capacity;        /* entries the arrays hold                */
    int64_t *count_dev;       /* int64: the number of live particles    */
    psamd_live_stats *stats_dev;
} psamd_export;

/* What psamd_inject did (see "putting particles in" below). */
typedef struct psamd_inject_result {
    int64_t done;             /* entries processed: n, or the index of the entry that stopped the call       */
    int64_t placed;           /* entries placed on THIS context (a slab places its own segments' entries)     */
    int32_t status;           /* PSAMD_OK, PSAMD_ERR_OUTSIDE_BOX or PSAMD_ERR_QUEUE_EMPTY: why it stopped     */
    int32_t reserved;
} psamd_inject_result;

/* What psamd_inject reads and where it writes (device pointers). */
typedef struct psamd_inject_spec {
    uint32_t flags;           /* 0 (reserved for later)                                                       */
    int32_t  reserved;        /* 0                                                                            */
    const void  *pos4;        /* float4[max_count] x, y, z, w -- required, 16-byte aligned                    */
    const void  *vel4;        /* float4[max_count] vx, vy, vz, age -- NULL: zeros; 16-byte aligned            */
    const float *fert_age;    /* float[max_count] -- NULL: 0                                                  */
    int64_t  max_count;       /* entries the arrays hold; sizes the launches; 0 <= max_count < 2^31           */
    const int64_t *count_dev; /* optional device int64: n = clamp(*count_dev, 0, max_count), read by the
                                 kernels; NULL: n = max_count                                                 */
    int32_t *ids_dev;         /* optional out, int32[max_count]: for every entry < n the slot id it was given,
                                 -1 if it was not placed here                                                 */
    psamd_inject_result *result_dev;   /* optional out (device); NULL: the context's own record only         */
} psamd_inject_spec;

/* What psamd_remove did (see "taking particles out" below). */
#define PSAMD_REMOVE_BOX     0x1u   /* the candidates are the live particles inside [lo, hi), not an id list          */
#define PSAMD_REMOVE_OUTSIDE 0x2u   /* with BOX only: the live particles NOT inside                                    */
typedef struct psamd_remove_result {
    int64_t done;             /* by id: n; by box: live owned particles examined                              */
    int64_t removed;          /* particles reset (outcomes 0 and 4)                                           */
    int64_t not_live, foreign, invalid;   /* by id: entries with the outcomes 1, 2, 3; by box: 0              */
    int64_t dropped;          /* of `removed`, slots a full queue did not take (outcome 4)                    */
} psamd_remove_result;        /* 48 bytes */

/* What psamd_remove reads and where it writes (device pointers). */
typedef struct psamd_remove_spec {
    uint32_t flags;           /* 0: by id; PSAMD_REMOVE_BOX [| PSAMD_REMOVE_OUTSIDE]: by box                  */
    int32_t  reserved;        /* 0                                                                            */
    const int32_t *ids;       /* by id: int32[max_count] slot ids, 4-byte aligned; required if max_count > 0  */
    int64_t  max_count;       /* by id: entries the arrays hold; sizes the launches; 0 <= max_count < 2^31    */
    const int64_t *count_dev; /* by id, optional device int64: n = clamp(*count_dev, 0, max_count), read by
                                 the kernels; NULL: n = max_count                                             */
    int32_t *outcome_dev;     /* by id, optional out, int32[max_count]: every entry's outcome code            */
    float    lo[3], hi[3];    /* by box: inside is lo.x <= x < hi.x, and likewise y and z, in fp32            */
    psamd_remove_result *result_dev;   /* optional out (device), 8-byte aligned; NULL: the context's own record only */
} psamd_remove_spec;          /* 72 bytes */

/* What psamd_potential found (see "energy" below). */
typedef struct psamd_potential_result {
    int64_t listed;           /* particles phi was formed for                                                 */
    int64_t nonfinite;        /* of them, with a phi that is not finite                                       */
    double  potential;        /* U                                                                            */
    double  phi_min, phi_max; /* over the finite ones; +inf / -inf if there is none                           */
} psamd_potential_result;     /* 40 bytes */

/* psamd_potential_spec.flags.  PSAMD_POTENTIAL_FAR: on a PSAMD_FLAG_FAR_MONOPOLE / PSAMD_FLAG_FAR_PYRAMID context, phi over
 * the stencil AND the far bodies of the context's force model (see "energy" below).  The bit exists so that a caller
 * written for "exactly the stencil's bodies" is never silently handed another quantity: without it such a context
 * refuses, with it the caller has said which phi it wants.  An unknown bit on every other context. */
#define PSAMD_POTENTIAL_FAR 0x1u
/* A modifier of PSAMD_POTENTIAL_FAR on a PSAMD_FLAG_FAR_QUADRUPOLE context: every far body also adds its quadrupole term, so
 * that phi is the potential of the field that context applies.  PSAMD_POTENTIAL_FAR alone was documented as "each far body as
 * one body (X, Y, Z, M)" and stays that promise: the quadrupole form is asked for by name, and without this bit such a context
 * refuses.  An unknown bit on every other context; without PSAMD_POTENTIAL_FAR PSAMD_ERR_INVALID_ARG. */
#define PSAMD_POTENTIAL_QUADRUPOLE 0x2u

/* What psamd_potential writes and where (device pointers). */
typedef struct psamd_potential_spec {
    uint32_t flags;           /* 0, or PSAMD_POTENTIAL_FAR on a far-monopole context (| PSAMD_POTENTIAL_QUADRUPOLE
                                 on a quadrupole context)                                                     */
    int32_t  reserved;        /* 0                                                                            */
    float   *phi;             /* optional out, float[capacity], 4-byte aligned; required if capacity > 0      */
    int64_t  capacity;        /* entries phi holds                                                            */
    psamd_potential_result *result_dev;   /* optional out (device), 8-byte aligned; NULL: the context's own record only */
} psamd_potential_spec;       /* 32 bytes */

/* psamd_probe: which components of the field are wanted (see "the field at chosen points" below). */
#define PSAMD_PROBE_ACC 0x1u   /* out4.xyz = acceleration at the point            */
#define PSAMD_PROBE_PHI 0x2u   /* out4.w   = potential at the point               */
#define PSAMD_PROBE_FAR 0x4u   /* a modifier beside ACC and / or PHI, on a PSAMD_FLAG_FAR_MONOPOLE / PSAMD_FLAG_FAR_PYRAMID
                                  context: the field of the stencil AND the far bodies of the context's force model.  It
                                  exists for PSAMD_POTENTIAL_FAR's reason; an unknown bit on every other context */
#define PSAMD_PROBE_QUADRUPOLE 0x8u   /* a modifier of PSAMD_PROBE_FAR on a PSAMD_FLAG_FAR_QUADRUPOLE context: the far bodies'
                                  quadrupole terms too (PSAMD_POTENTIAL_QUADRUPOLE's rule); an unknown bit on every other
                                  context, PSAMD_ERR_INVALID_ARG without PSAMD_PROBE_FAR */

/* What psamd_probe did. */
typedef struct psamd_probe_result {
    int64_t done;             /* n: entries examined                                                          */
    int64_t served;           /* outcome 0                                                                    */
    int64_t outside;          /* outcome 1                                                                    */
    int64_t foreign;          /* outcome 2                                                                    */
    int64_t nonfinite;        /* of `served`, entries with a requested component not finite                   */
} psamd_probe_result;         /* 40 bytes */

/* What psamd_probe reads and where it writes (device pointers). */
typedef struct psamd_probe_spec {
    uint32_t fields;          /* PSAMD_PROBE_ACC | PSAMD_PROBE_PHI, at least one; PSAMD_PROBE_FAR (and
                                 PSAMD_PROBE_QUADRUPOLE) beside them                                          */
    int32_t  reserved;        /* 0                                                                            */
    const void *pos4;         /* float4[max_count] x, y, z (w ignored), 16-byte aligned: an export's pos4 can
                                 be passed as it is                                                           */
    int64_t  max_count;       /* 0 <= max_count < 2^31; sizes the launches                                    */
    const int64_t *count_dev; /* optional device int64: n = clamp(*count_dev, 0, max_count), read by the
                                 kernels; NULL: n = max_count                                                 */
    void    *out4;            /* float4[max_count], 16-byte aligned, not pos4; required if max_count > 0      */
    int32_t *outcome_dev;     /* optional out, int32[max_count]: every entry's outcome code                   */
    psamd_probe_result *result_dev;   /* optional out (device), 8-byte aligned; NULL: the context's own record only */
} psamd_probe_spec;           /* 56 bytes */

/* psamd_update: which words of a particle an entry carries (see "changing particles in place" below). */
#define PSAMD_UPDATE_VEL   0x1u    /* vel4[k].xyz -> the particle's vx, vy, vz                          */
#define PSAMD_UPDATE_AGE   0x2u    /* vel4[k].w   -> age                                                */
#define PSAMD_UPDATE_MASS  0x4u    /* w[k]        -> w (pos4.w; x, y, z keep their bits)                */
#define PSAMD_UPDATE_FERT  0x8u    /* fert_age[k] -> fertility age (acc4.w; ax, ay, az keep their bits) */
#define PSAMD_UPDATE_ADD          0x100u  /* modifier of VEL: v = RN(v + vel4[k]) per component, fp32, one rounding, no clamp (a kick) */
#define PSAMD_UPDATE_EXPORT_ORDER 0x200u  /* entry k belongs to the k-th live owned particle in ascending slot id; ids must be NULL    */

/* What psamd_update did. */
typedef struct psamd_update_result {
    int64_t done;             /* n: entries examined                                                          */
    int64_t updated;          /* outcome 0                                                                    */
    int64_t not_live, foreign, invalid, duplicate;   /* outcomes 1, 2, 3, 4                                   */
} psamd_update_result;        /* 48 bytes */

/* What psamd_update reads and where it writes (device pointers; none of them inside the context's own arrays). */
typedef struct psamd_update_spec {
    uint32_t fields;          /* PSAMD_UPDATE_VEL | _AGE | _MASS | _FERT, at least one; PSAMD_UPDATE_ADD and
                                 PSAMD_UPDATE_EXPORT_ORDER beside them                                         */
    int32_t  reserved;        /* 0                                                                            */
    const int32_t *ids;       /* by id: int32[max_count] slot ids, 4-byte aligned, required if max_count > 0;
                                 NULL with PSAMD_UPDATE_EXPORT_ORDER                                          */
    const void    *vel4;      /* float4[max_count] vx, vy, vz, age, 16-byte aligned; required with VEL or AGE
                                 (if max_count > 0); ignored otherwise                                        */
    const float   *w;         /* float[max_count]; required with MASS, ignored otherwise                      */
    const float   *fert_age;  /* float[max_count]; required with FERT, ignored otherwise                      */
    int64_t  max_count;       /* entries the arrays hold; sizes the launches; 0 <= max_count < 2^31           */
    const int64_t *count_dev; /* optional device int64: n = clamp(*count_dev, 0, max_count), read by the
                                 kernels; NULL: n = max_count                                                 */
    int32_t *outcome_dev;     /* optional out, int32[max_count]: every entry's outcome code                   */
    psamd_update_result *result_dev;   /* optional out (device), 8-byte aligned; NULL: the context's own record only */
} psamd_update_spec;          /* 72 bytes */

/* What psamd_deposit did (see "mass on a lattice" below). */
typedef struct psamd_deposit_result {
    int64_t voxels;           /* voxels this context wrote                                                    */
    int64_t bodies;           /* listed finite bodies of this context's served cells                          */
    int64_t skipped;          /* listed bodies of those cells with a non-finite word                          */
    double  mass;             /* fp64 sum of this context's voxel sums (before the float rounding), fixed order */
    double  vmax;             /* largest voxel value written; -inf if none                                    */
} psamd_deposit_result;       /* 40 bytes */

/* What psamd_deposit writes and where (device pointers). */
typedef struct psamd_deposit_spec {
    uint32_t flags;           /* 0                                                                            */
    int32_t  refine;          /* k: voxels per cell edge, 1, 2 or 4                                           */
    float   *out;             /* float[capacity], 4-byte aligned, required                                    */
    int64_t  capacity;        /* >= (grid_dim * refine)^3                                                     */
    psamd_deposit_result *result_dev;  /* optional out (device), 8-byte aligned; NULL: the context's own record only */
} psamd_deposit_spec;         /* 32 bytes */

/* psamd_sample_spec.flags (see "a lattice field at the particles" below) */
#define PSAMD_SAMPLE_VEC4         0x1u  /* field is float4 per voxel, out is float4 per entry; without it float / float */
#define PSAMD_SAMPLE_EXPORT_ORDER 0x2u  /* pos4 must be NULL: entry k is the k-th live owned particle in ascending global
                                           slot id (psamd_export_live's pairing); its x, y, z come from the context */

/* What psamd_sample did. */
typedef struct psamd_sample_result {
    int64_t done;             /* n: entries examined                                                          */
    int64_t served;           /* outcome 0                                                                    */
    int64_t outside;          /* outcome 1                                                                    */
    int64_t nonfinite;        /* of served, entries with a word of out not finite                             */
} psamd_sample_result;        /* 32 bytes */

/* What psamd_sample reads and where it writes (device pointers; none of them inside the context's own arrays). */
typedef struct psamd_sample_spec {
    uint32_t flags;           /* PSAMD_SAMPLE_*                                                               */
    int32_t  refine;          /* k: 1, 2 or 4 -- psamd_deposit's lattice                                      */
    const void *field;        /* float[capacity] or float4[capacity], indexed as psamd_deposit's out; required */
    int64_t  capacity;        /* >= (grid_dim * refine)^3 voxels                                              */
    const void *pos4;         /* float4[max_count], x, y, z (w ignored); NULL with PSAMD_SAMPLE_EXPORT_ORDER  */
    int64_t  max_count;       /* 0 <= max_count < 2^31; sizes the launches                                    */
    const int64_t *count_dev; /* optional, 8-byte aligned: n = clamp(*count_dev, 0, max_count), read by the
                                 kernels; NULL: n = max_count                                                 */
    void    *out;             /* float[max_count] or float4[max_count]                                        */
    float    scale;           /* every word of out is RN(scale * value); taken as given (0 gives zeros)       */
    int32_t  reserved;        /* 0                                                                            */
    int32_t *outcome_dev;     /* optional out, int32[max_count]: every entry's outcome code                   */
    psamd_sample_result *result_dev;   /* optional out (device), 8-byte aligned; NULL: the context's own record only */
} psamd_sample_spec;          /* 80 bytes */

/* psamd_neighbours_spec.flags (see "neighbours within a radius" below) */
#define PSAMD_NEIGHBOURS_INDEX 0x1u     /* a neighbour is named by its export index, not by its global slot id (world == 1) */

/* What psamd_neighbours found. */
typedef struct psamd_neighbours_result {
    int64_t listed;           /* the queries: the particles of the own cells' lists                           */
    int64_t pairs;            /* the sum of all queries' counts, the whole context's: directed pairs          */
    int64_t wanted;           /* offsets[m]: the list entries the first m = min(live, capacity) particles have */
    int32_t max_count;        /* the largest count                                                            */
    int32_t reserved;         /* 0                                                                            */
    double  d2_min;           /* the smallest d2 over all neighbours; +inf if there is none                   */
} psamd_neighbours_result;    /* 40 bytes */

/* What psamd_neighbours writes and where (device pointers; none of them inside the context's own arrays). */
typedef struct psamd_neighbours_spec {
    uint32_t flags;           /* PSAMD_NEIGHBOURS_*                                                           */
    float    radius;          /* finite, > 0, (double)radius <= cell_size                                     */
    int32_t *count;           /* optional out, int32[capacity], 4-byte aligned: neighbours; -1: in no list    */
    int32_t *nearest;         /* optional out, int32[capacity]: the neighbour with the smallest d2, or -1     */
    float   *nearest_d2;      /* optional out, float[capacity]: that d2, or +inf                              */
    int64_t *offsets;         /* optional out, int64[capacity + 1], 8-byte aligned: exclusive prefix of max(count, 0) */
    int64_t  capacity;        /* >= 0: entries of the export order that are written                           */
    int32_t *list;            /* optional out, int32[list_capacity]; needs offsets                            */
    int64_t  list_capacity;   /* >= 0: position p of the lists is written iff p < list_capacity               */
    psamd_neighbours_result *result_dev;   /* optional out (device), 8-byte aligned; NULL: the context's own record only */
} psamd_neighbours_spec;      /* 72 bytes */

/* psamd_groups_spec.flags (see "groups within a radius" below) */
#define PSAMD_GROUPS_INDEX 0x1u   /* group_first names a particle by its export index, not its global slot id */

/* What psamd_groups found. */
typedef struct psamd_groups_result {
    int64_t members;     /* particles that belong to a group (see Members) */
    int64_t groups;      /* the number of groups, singles included */
    int64_t links;       /* undirected member pairs with d2 <= r2 over the stencil */
    int64_t singles;     /* groups of one */
    int32_t largest;     /* the largest group's size; 0 if there is no member */
    int32_t unfinished;  /* unions that hit the step cap (see Bounded loops): 0, always, on correct code */
} psamd_groups_result;   /* 40 bytes */

/* What psamd_groups writes and where (device pointers; none of them inside the context's own arrays). */
typedef struct psamd_groups_spec {
    uint32_t flags;          /* PSAMD_GROUPS_* */
    float    radius;         /* psamd_neighbours' rule: finite, > 0, (double)radius <= cell_size */
    int32_t *group;          /* optional out, int32[capacity], export order: the dense group number g, -1: no member */
    int64_t  capacity;       /* >= 0 */
    int32_t *group_first;    /* optional out, int32[group_capacity]: group g's smallest member */
    int32_t *group_size;     /* optional out, int32[group_capacity]: group g's members */
    int64_t  group_capacity; /* >= 0: entry g of the two tables is written iff g < group_capacity */
    psamd_groups_result *result_dev;  /* optional out (device), 8-byte aligned */
} psamd_groups_spec;     /* 56 bytes */

/* psamd_knn_spec.flags (see "the k nearest within a radius" below) */
#define PSAMD_KNN_INDEX 0x1u      /* a neighbour is named by its export index, not its global slot id (world == 1) */
#define PSAMD_KNN_MAX_K 32

/* What psamd_knn found. */
typedef struct psamd_knn_result {
    int64_t listed;     /* the queries: psamd_neighbours' */
    int64_t found;      /* the sum over the queries of min(count, k) */
    int64_t full;       /* queries with count >= k */
    int32_t k, reserved;
    double  dk2_min, dk2_max;   /* smallest / largest d2 of a k-th neighbour over the full queries; +inf / -inf if none */
} psamd_knn_result;     /* 48 bytes */

/* What psamd_knn writes and where (device pointers; none of them inside the context's own arrays). */
typedef struct psamd_knn_spec {
    uint32_t flags;     /* PSAMD_KNN_* */
    float    radius;    /* psamd_neighbours' rule: finite, > 0, (double)radius <= cell_size */
    int32_t  k;         /* 1 .. PSAMD_KNN_MAX_K */
    int32_t  reserved;  /* 0 */
    int32_t *found;     /* optional out, int32[capacity]: min(count, k); -1: in no list of the frame */
    int32_t *who;       /* optional out, int32[capacity * k], row-major: entry o's j-th nearest at who[o * k + j] */
    float   *d2;        /* optional out, float[capacity * k]: that pair's d2 */
    int64_t  capacity;  /* >= 0: entries of the export order that are written */
    psamd_knn_result *result_dev;   /* optional out (device), 8-byte aligned */
} psamd_knn_spec;       /* 56 bytes */

typedef struct psamd_ctx psamd_ctx;

/* ---- lifetime ------------------------------------------------------------ */
int         psamd_abi_version(void);
const char *psamd_status_string(int status);
int         psamd_default_config(psamd_config *cfg);
/* DoInit + init_particles + q_start_fast + pkg_distrib (ps.cpp:2200-2235,
 * 722-753, 814-871, 893-911): allocates the container, marks every slot free. */
int         psamd_create(const psamd_config *cfg, psamd_ctx **out);
int         psamd_destroy(psamd_ctx *ctx);
const char *psamd_last_error(const psamd_ctx *ctx);
int         psamd_get_sizes(const psamd_ctx *ctx, psamd_sizes *out);
int         psamd_get_config(const psamd_ctx *ctx, psamd_config *out);

/* ---- host-only geometry (no device needed) ------------------------------------------ */
/* What DoInit and the one-off setup stages derive from a configuration, computed on the
 * host without touching a GPU: sizes (ps.cpp:2204-2222), the cell -> (chunk, seg_type,
 * seg_tid) table (get_cell_info), the chunk package table (set_pkg_segments) and the
 * initial free-slot queues (q_start_fast).  Any output pointer may be NULL. */
int psamd_describe(const psamd_config *cfg, psamd_sizes *sizes, int32_t *cell_table3,
                   int32_t *pkgdistrib_pairs, void *queue_info24, int32_t *queue);

/* ---- setup stage: fill_particles, task 5 (ps.cpp:915-1048) --------------- */
/* Places n particles in order; each takes the next free slot of its segment
 * (q_remove) and is initialised as create_particle_s does (app.cu:189-208).
 * w / age / fert_age may be NULL => particle_weight / 0 / 0.  ids_out (may be
 * NULL) receives the slot ids.  On error nothing after the failing particle is
 * placed and *n_done (may be NULL) says how many were. */
int psamd_fill_particles(psamd_ctx *ctx, int64_t n, const float *xyz, const float *vxyz,
                         const float *w, const float *age, const float *fert_age,
                         int32_t *ids_out, int64_t *n_done);
/* The reference's own initial distribution (ps.cpp:974-1028) with a fixed seed in
 * place of std::random_device: n points uniform in the box, written to xyz_out. */
int psamd_uniform_cloud(const psamd_ctx *ctx, int64_t n, uint32_t seed, float *xyz_out);

/* ---- the reference's buffers, in the reference's own layouts -------------- */
/* P_DATA_TYPE[count] (72-byte records, common.h:94-120) for slots first..first+count-1 */
int psamd_upload_particles(psamd_ctx *ctx, const void *p72, int64_t first, int64_t count);
int psamd_download_particles(psamd_ctx *ctx, void *p72, int64_t first, int64_t count);
/* T_DATA_TYPE[count] (24-byte records, common.h:122-132): the build_grid snapshot.  Inside the library the rows are a
 * MIRROR kept for this call: nothing in the step reads them (the pair stage reads its own sorted snapshot, gathered
 * from the particle arrays).  A host that never fetches T_DATA switches the mirror off -- psamd_set_tdata_mirror(ctx, 0):
 * build_grid then leaves the rows alone (56 bytes of traffic per particle and step less) and this call returns
 * PSAMD_ERR_STATE; switching it on again makes the rows exact from the next build_grid on for the slots alive then
 * (rows of slots that were alive only while it was off keep their older contents).  Default: on. */
int psamd_download_tdata(psamd_ctx *ctx, void *t24, int64_t first, int64_t count);
int psamd_set_tdata_mirror(psamd_ctx *ctx, int enabled);
/* QUEUE_INFO[queue_info_size] + int[container_size] (common.h:134-139, ps.cpp:72-73) */
int psamd_upload_queues(psamd_ctx *ctx, const void *queue_info24, const int32_t *queue);
int psamd_download_queues(psamd_ctx *ctx, void *queue_info24, int32_t *queue);
/* int[n_cellgrid] / int[n_chunkgrid], element 0 of each row = count (ps.cpp:1502-1516) */
int psamd_download_cellgrid(psamd_ctx *ctx, int32_t *out);
int psamd_download_chunkgrid(psamd_ctx *ctx, int32_t *out);
/* int[num_cells]: per cell, the particles the last pair pass computed a force for (those the
 * reference's force loop runs for, ps.cpp:1242-1263: no collision this step, not a kid).
 * Valid after psamd_calc_forces_pairs of the same frame. */
int psamd_download_force_counts(psamd_ctx *ctx, int32_t *out);
/* PAIR[num_chunks*27] (app_common.cu:150-232) and the cell -> (chunk, seg_type,
 * seg_tid) table (get_cell_info, app_common.cu:50-148), 3 ints per cell */
int psamd_get_pkgdistrib(const psamd_ctx *ctx, int32_t *pairs_out);
int psamd_get_cell_table(const psamd_ctx *ctx, int32_t *out3_per_cell);
/* hostGridMax: [0] biggest chunk, [1] biggest cell (ps.cpp:76, read at ps.cpp:1900) */
int psamd_get_gridmax(psamd_ctx *ctx, int32_t out2[2]);

/* ---- the three per-step stages ------------------------------------------ */
int psamd_init_iframe(psamd_ctx *ctx);  /* task 3, ps.cpp:1574-1606 / psCUDA.cu:104-150 */
int psamd_build_grid(psamd_ctx *ctx);   /* task 8, ps.cpp:1468-1537 / psCUDA.cu:442-499 */
int psamd_calc_forces(psamd_ctx *ctx);  /* task 6, ps.cpp:1120-1383 / psCUDA.cu:152-423 */
/* calc_forces in its two halves: _pairs computes every particle's collision flag and acceleration
 * (ps.cpp:1182-1263) and leaves the acceleration where the particle keeps it -- T_DATA's ax, ay, az, as
 * the reference's thread does at ps.cpp:1300-1302 -- and the flag beside it (psamd_download_force4 reads
 * both back in the cell-sorted order); _apply does everything after the two neighbour loops (kill /
 * survive / integrate / explosion / relocation, ps.cpp:1210-1374).  psamd_calc_forces == _pairs then
 * _apply; between the two a download of the particles shows the new accelerations beside the old
 * positions and velocities. */
int psamd_calc_forces_pairs(psamd_ctx *ctx);
int psamd_calc_forces_apply(psamd_ctx *ctx);
/* nsteps x {init_iframe, build_grid, calc_forces}, enqueued on the context's stream.  NOTHING in a step waits
 * for the host: the step's one read-back (live count, sticky error bits, list sizes -- what the reference's driver
 * fetches as hostGridMax, ps.cpp:1878-1900) lands in a pinned host record that the library reads ONE STEP LATE.
 * A stage call therefore returns the verdict of the steps BEFORE the one it has just enqueued (run-ahead 1, the
 * default: the host stays a step ahead of the GPU and is never on the step's critical path); psamd_synchronize
 * waits for everything enqueued and returns whatever verdict is outstanding.  psamd_set_run_ahead(ctx, 0): every
 * call that ends a step (psamd_step, psamd_calc_forces[_apply], psamd_slab_finish) waits for that step's own
 * record before it returns, as the reference's driver waits for its task (ps.cpp:1716).  Calls that hand buffers or
 * counters to the caller synchronise by themselves.  If a step's record does not arrive within 10 s (environment
 * PSAMD_WAIT_LIMIT_S) while its stream stays busy, the call returns PSAMD_ERR_STATE and the context refuses all
 * further work: a wedged GPU is reported, not waited for. */
int psamd_step(psamd_ctx *ctx, int32_t nsteps);
int psamd_synchronize(psamd_ctx *ctx);
int psamd_set_run_ahead(psamd_ctx *ctx, int steps);   /* 0 or 1 */

/* float4 (ax, ay, az, flag-as-int-bits) entries [first, first+count) of the sorted-order
 * force array (diagnostics). */
int psamd_download_force4(psamd_ctx *ctx, void *out_float4, int64_t first, int64_t count);

/* ---- checkpoint / resume --------------------------------------------------------- */
/* The reference keeps its whole state in the nine buffers; the
 * device-side image of them (particles + free-slot queues) can be saved once and
 * restored any number of times without leaving HBM. */
int psamd_snapshot_save(psamd_ctx *ctx);
int psamd_snapshot_restore(psamd_ctx *ctx);

/* ---- slab partition (multi-GPU) ---------------------------------------------------- */
/* The reference distributes by segment: a chunk subtask subscribes to its interior segment
 * and the 26 face / edge / corner segments around it (ps.cpp:380-487, set_pkg_segments
 * app_common.cu:150-232), each one contiguous slot range with its own free-slot queue.
 * Here the same segments are dealt to the GPUs of a node in slabs of cell layers along i3
 * (the slowest cell index, so a slab is one contiguous run of the cell-major order):
 *   - STATE layers: the segments whose particles, slots and queues live on the rank.  The
 *     reference numbers segments plane by plane, so a rank owns one slot range and one run of
 *     QUEUE_INFO records per segment type.  Every queue has exactly one owner, which replays
 *     its operations in the reference's serial order.
 *   - COMPUTE layers: the cells whose collision flags and forces the rank evaluates; cut for
 *     balance, anywhere.  Where a cut falls inside a segment group, the upper layers are
 *     computed by the rank above ("lent"): their snapshot travels up with the halo layer and
 *     their (ax, ay, az, flag) records come back before the owner integrates.
 * Per step a rank exchanges, with its two neighbours only: the snapshot (x, y, z, mass, age,
 * id) of its boundary layers; the force records of lent layers; and the particles whose new
 * segment belongs to the neighbour (periodic box: the ring closes), keyed so that the
 * neighbour's queue hands out their slots in the reference's order.  Nothing is replicated
 * but the O(cells) tables.  Message sizes are known to both ends without a word between them (fixed by the plan;
 * the transfer messages grow by a rule every rank evaluates on the same all-gathered numbers); the transport (RCCL
 * send/recv on device memory, or anything else) is the caller's: see particlesystem_amd/slab.py. */
typedef struct psamd_slab_plan {
    int32_t world, rank, grid_dim;
    int32_t cut_lo, cut_hi;          /* compute layers [lo, hi)                                  */
    int32_t state_lo, state_hi;      /* layers whose particles live here                         */
    int32_t below_lo, below_hi;      /* layers received from rank-1: halo layer, then lent layers */
    int32_t above_lo, above_hi;      /* halo layer received from rank+1 (group-aligned cut only)  */
    int32_t lentin_lo, lentin_hi;    /* the part of `below` this rank computes for rank-1         */
    int32_t lentout_lo, lentout_hi;  /* own layers computed by rank+1                             */
    int32_t send_up_lo, send_up_hi;      /* own layers whose snapshot goes to rank+1              */
    int32_t send_down_lo, send_down_hi;  /* own layers whose snapshot goes to rank-1              */
    int32_t slot_lo[4], slot_hi[4];  /* owned slot range per segment type (1, 2, 4, 8)            */
    int32_t rec_lo[4], rec_hi[4];    /* owned QUEUE_INFO records per segment type                 */
    int32_t up_rank, down_rank;      /* ring neighbours for particles that change owner; -1: none */
} psamd_slab_plan;
/* host only, no device needed: the plan of cfg->rank in a world of cfg->world ranks */
int psamd_slab_plan_describe(const psamd_config *cfg, psamd_slab_plan *out);
int psamd_get_slab_plan(const psamd_ctx *ctx, psamd_slab_plan *out);

/* Message buffers (device memory owned by the context; bytes = 0: this rank has no such
 * message).  Index 0 = the neighbour below (rank-1), 1 = the neighbour above (rank+1). */
typedef struct psamd_slab_buffers {
    void   *halo_out[2], *halo_in[2];      /* layer snapshots                                    */
    int64_t halo_out_bytes[2], halo_in_bytes[2];
    void   *force_out, *force_in;          /* force records of lent layers: out to rank-1, in from rank+1 */
    int64_t force_out_bytes, force_in_bytes;
    void   *xfer_out[2], *xfer_in[2];      /* particles changing owner (ring: down_rank / up_rank) */
    int64_t xfer_bytes;                    /* all four the same size: what to post THIS step -- it may change from step to step, on
                                              every rank in the same step (config.xfer_cap_max); read it after psamd_slab_apply */
    void   *status_out, *status_in;        /* ALL-GATHERED once per step: status_in = world records of status_bytes each, by rank */
    int64_t status_bytes;
    void   *allg_out, *allg_in;            /* ALL-GATHERED once per step between slab_build and slab_pairs; allg_in = world blocks of
                                              allg_bytes, by rank.  PSAMD_FLAG_ALL_PAIRS: the snapshot (x, y, z, w_eff) of every rank's
                                              own cells.  PSAMD_FLAG_FAR_SLAB: the fp64 sums of every rank's own cells ("far field on
                                              slabs" below).  Every other context: 0 bytes */
    int64_t allg_bytes;
    void   *xfer2_out[2], *xfer2_in[2];    /* same exchange as xfer_*, but between ranks TWO apart on the ring: out[0] -> rank-2's in[1],
                                              out[1] -> rank+2's in[0].  Only in worlds (>= 4 ranks) where some rank's whole state is one
                                              cell layer, which a particle crossing two layers in a step can fly over; else 0 bytes */
    int64_t xfer2_bytes;
    void   *far_out, *far_in;              /* ALL-GATHERED in the transfer phase (with xfer_*): records for a rank further away than the
                                              neighbour messages reach; far_in = world blocks of far_bytes, by rank.  A particle whose
                                              position stopped being a number is filed under one fixed cell wherever it was (the
                                              reference's conversion): only births make such particles, so the buffers exist in worlds
                                              of >= 4 ranks with PSAMD_FLAG_EXPLOSIONS; else 0 bytes */
    int64_t far_bytes;
    int64_t xfer_bytes_max;                /* the room of the xfer_* buffers: xfer_bytes never grows beyond it (config.xfer_cap_max) */
} psamd_slab_buffers;
int psamd_slab_buffers_get(psamd_ctx *ctx, psamd_slab_buffers *out);

/* One step = build, [all-gather status_out into every rank's status_in -- it must have landed before the
 * FIRST pair-stage call, pairs_interior where that is used: the stage writes the particles' new accelerations
 * into their records and has to know whom the chunk lists' capacity rule takes out of the step;
 * exchange halo_out -> neighbours' halo_in; with PSAMD_FLAG_ALL_PAIRS or PSAMD_FLAG_FAR_SLAB the all-gather of
 * allg_out into allg_in, which must have landed], pairs, [force_out -> rank-1's force_in], apply, [xfer_out -> neighbours' xfer_in; where they exist xfer2_* likewise and the all-gather of far_out into far_in], finish.  The status record carries a rank's
 * sticky error bits, the slots the cell-overflow rule killed, which the reference frees into queue
 * record 0 wherever they were (ps.cpp:1523-1526), and the rank's part of every chunk's particle count
 * per segment type, from which all ranks reproduce the chunk lists' capacity rule (ps.cpp:1502-1508)
 * and hostGridMax[0].  A slab fails COLLECTIVELY: slab_finish returns an error only for error bits
 * that were in a step's status records, which all ranks see alike -- with run-ahead 1 (the default) from the
 * slab_finish of the step AFTER, on every rank alike; an error raised after a rank's
 * record was closed goes out with the next step's record and stops every rank there (or is reported by
 * psamd_synchronize).  All asynchronous on the context's stream.  With world == 1
 * the four calls are psamd_step(1) cut in four and no message exists; with world == 1 a frame is stepped by one
 * family of calls -- these, or init_iframe / build_grid / calc_forces / step -- from its build to its end. */
int psamd_slab_build(psamd_ctx *ctx);   /* init_iframe + build_grid of the own layers; packs halo_out   */
int psamd_slab_pairs_interior(psamd_ctx *ctx);  /* optional, while the halo travels: the pair stage of the cells whose
                                                    stencil lies in the rank's own layers (needs the status records only) */
int psamd_slab_pairs(psamd_ctx *ctx);   /* unpacks halo_in; collision flags + forces (of the remaining cells); packs force_out */
int psamd_slab_apply(psamd_ctx *ctx);   /* unpacks force_in; integrate ... (calc_forces' tail); closes xfer_out */
int psamd_slab_finish(psamd_ctx *ctx);  /* merges xfer_in; queue replay and relocation                  */
/* Transport through host memory (tests, two processes sharing one GPU): copy message buffer
 * `which` to / from the host.  which: 0/1 halo_out[0/1], 2/3 halo_in[0/1], 4 force_out,
 * 5 force_in, 6/7 xfer_out[0/1], 8/9 xfer_in[0/1], 10 status_out, 11 status_in, 12 allg_out, 13 allg_in,
 * 14/15 xfer2_out[0/1], 16/17 xfer2_in[0/1], 18 far_out, 19 far_in. */
int psamd_slab_msg_download(psamd_ctx *ctx, int which, void *host, int64_t bytes);
int psamd_slab_msg_upload(psamd_ctx *ctx, int which, const void *host, int64_t bytes);

/* Enqueue all further work on the caller's HIP stream (e.g. the one RCCL orders
 * against) instead of the context's own.  NULL restores the context's stream. */
int psamd_set_stream(psamd_ctx *ctx, void *hip_stream);
/* the HIP stream the context enqueues on now (its own unless psamd_set_stream gave it another) */
int psamd_get_stream(psamd_ctx *ctx, void **hip_stream_out);

/* One submission per stage sequence: with graphs on, the kernels a stage call enqueues (psamd_slab_build / _pairs /
 * _apply / _finish up to its read-back; psamd_step: init_iframe .. the queue replay) are captured into a hipGraph the
 * first time a launch shape is met and replayed afterwards -- a rank's step is then four or five submissions instead of
 * two dozen launches.  The results are the same kernels' (tests compare every byte with graphs on); steps that carry
 * timing events run eagerly.  Nothing a graph replays depends on the step: sizes, the step's number and the sequence
 * number of the scalar record live in device memory.  psamd_get_graph_stats: replays and captures so far; returns
 * PSAMD_ERR_UNSUPPORTED (and says why) if the runtime refused a capture and the context fell back to plain launches. */
int psamd_set_graphs(psamd_ctx *ctx, int enabled);
int psamd_get_graph_stats(psamd_ctx *ctx, int64_t *launches, int64_t *captures);
/* How the calling thread waits for a step's scalars when it has to (the one read-back of a step, ps.cpp:1878-1900;
 * with run-ahead the record is there long before it is asked for): 0 spins on the
 * pinned record (default of a single context: lowest latency), 1 spins for a few microseconds and then sleeps in
 * 5-us naps (default of a slab: a node's eight ranks do not pin eight cores).  While it naps the library lowers the
 * calling thread's timer slack (prctl PR_SET_TIMERSLACK) to 1 us and restores the old value before the call returns. */
int psamd_set_wait_policy(psamd_ctx *ctx, int policy);

/* ---- getting frames out ---------------------------------------------------- */
/* The live particles (0 <= cell < num_cells, what psamd_live_count counts; the mid-step encodings cell <= -2 are not
 * live) as compact arrays in ascending global slot id, one array per field, with their count and statistics: a frame
 * for a renderer, an analysis or a checkpoint, without the whole container (psamd_download_particles packs every slot,
 * free ones included, into 72-byte records).  The first min(count, capacity) live particles are written; the count
 * is always the full one.  Entry k equals, field for field and bit for bit, the k-th record of
 * psamd_download_particles filtered by the same predicate at the same point of the stream.
 *
 * psamd_export_live: enqueued on the context's stream (psamd_get_stream) and nothing else -- it allocates nothing,
 * waits for nothing and reads nothing back, so it may be captured into a graph.  It sees the state that the work
 * enqueued before it leaves behind: after psamd_step(ctx, n) it sees step n, also with run-ahead 1 and graphs on.
 * The arrays, *count_dev and *stats_dev are written by the time the stream reaches the end of the export.  The
 * launches cover every owned slot; the cost is about two passes over the live particles' fields plus the cell array.
 * PSAMD_ERR_INVALID_ARG: a NULL context or spec, unknown field bits, reserved != 0, capacity < 0, or a field asked for
 * with a NULL or misaligned pointer.  PSAMD_ERR_STATE: the context is wedged.
 *
 * A slab (world > 1) exports its own slots, with their global ids; the union of the ranks' exports sorted by id is
 * the export of one context that holds the whole system, and psamd_live_stats of the ranks combine by adding the
 * counts and sums and taking the minima and maxima (sums then agree to rounding, not to the bit).
 *
 * psamd_download_live: the same into host arrays (`capacity` entries each, a NULL pointer where the field is not
 * asked for); only the min(count, capacity) entries cross PCIe.  *count (required) = the full count.  Waits for the
 * context's stream.
 * psamd_live_stats_get: the statistics alone, into host memory; waits for the context's stream. */
int psamd_export_live(psamd_ctx *ctx, const psamd_export *spec);
int psamd_download_live(psamd_ctx *ctx, uint32_t fields, void *pos4, void *vel4, void *acc4, int32_t *id,
                        int32_t *cell, int64_t capacity, int64_t *count);
int psamd_live_stats_get(psamd_ctx *ctx, psamd_live_stats *out);

/* ---- putting particles in ------------------------------------------------- */
/* psamd_inject: the device-side, stream-ordered psamd_fill_particles.  Entries [0, n) are placed with xyz = pos4.xyz,
 * w = pos4.w, vxyz = vel4.xyz, age = vel4.w and fert_age, at the point of the stream where the call is made, and leave
 * the same bytes fill leaves when called there with the same particles: the particle arrays, the queues and their
 * QUEUE_INFO records, the ids, `done` (fill's *n_done), `placed` and the status.  Each entry takes the next free slot
 * of its segment's queue, in entry order (q_remove), and the slot is written as create_particle_s writes it
 * (acceleration 0, fertility age, not a parent).  A slab (world > 1) places only the entries whose segment record it
 * owns; the others get id -1 and count in `done`, not in `placed` -- every rank is given all entries and keeps its own.
 *
 * The call stops at the first failure, as fill does: an entry outside the box (what Geometry::locate rejects: the
 * fp64 floor((+-1.0 * c) / cell_size) + G / 2 range test, non-finite and huge coordinates included) stops it at its
 * index with PSAMD_ERR_OUTSIDE_BOX; an owned entry whose segment's queue is empty at its turn stops it at its index with
 * PSAMD_ERR_QUEUE_EMPTY; nothing at or after that index is placed.  Only the result record reports the stop: the call
 * returns PSAMD_OK once the work is enqueued, and the context carries on.
 *
 * Everything is enqueued on the context's stream: nothing waits and nothing is read back.  Scratch for the entries is
 * allocated when max_count exceeds what an earlier call allocated for (that growth may wait for the device); steady
 * use neither allocates nor waits.  Like fill, the call ends a frame in progress: psamd_calc_forces refuses with
 * PSAMD_ERR_STATE until psamd_build_grid runs again.  The host's bound of the live count (what sizes the all-pairs far
 * pass) grows by max_count at the call, also across steps enqueued before it whose records the host has yet to read.
 * Because of that bookkeeping the call is refused while the context's stream is being captured (PSAMD_ERR_STATE): a
 * replayed graph would inject without it.
 *
 * PSAMD_ERR_INVALID_ARG: a NULL context or spec, flags or reserved not 0, max_count out of range, pos4 NULL or not
 * 16-byte aligned, vel4 not 16-byte aligned, fert_age or ids_dev not 4-byte aligned, count_dev or result_dev not
 * 8-byte aligned.  PSAMD_ERR_STATE: the context is wedged, or its stream is being captured.  max_count == 0 writes a
 * zero result and launches nothing else.
 *
 * psamd_inject_result_get: the last inject's record, into host memory; waits for the context's stream. */
int psamd_inject(psamd_ctx *ctx, const psamd_inject_spec *spec);
int psamd_inject_result_get(psamd_ctx *ctx, psamd_inject_result *out);

/* ---- taking particles out -------------------------------------------------- */
/* psamd_remove: the device-side, stream-ordered counterpart of the reference's kill (reset_particle, then q_insert of
 * the slot id into the queue of the slot's own segment: ps.cpp:1210-1242).  A set of candidate slots is processed in a
 * defined serial order.  A candidate whose slot is live at its turn (0 <= cell < num_cells, what psamd_live_count counts)
 * is removed: the slot becomes a free slot's record (cell -1, position, velocity, acceleration and flags zero) and its id
 * goes to the rear of the queue of the segment the SLOT belongs to (get_id_info of the id, not the particle's cell),
 * exactly as q_insert does it: an empty record restarts at front = rear = rloc whatever the two held, rear wraps from
 * rloc + seg_size - 1 to rloc, and a record with count == seg_size takes nothing -- the particle is reset all the same
 * and counts in `dropped` (the cell-overflow rule frees foreign slots into record 0, so a queue can be full while one of
 * its slots is live).  After the call psamd_download_particles and psamd_download_queues return, byte for byte, what the
 * reference's serial reset + q_insert over the same candidates leave, and the steps that follow stay equal.  T_DATA
 * mirror rows are not touched (the reference's reset does not touch them either).
 *
 * By id (flags == 0): the candidates are the entries [0, n) of `ids`, in entry order.  Every entry gets an outcome,
 * written to outcome_dev if given:
 *     0  removed
 *     1  the slot is not live at the entry's turn -- a free slot, and the second and later occurrences of a
 *        duplicated id (that is the whole duplicate rule)
 *     2  a valid id whose slot this context does not own (a slab is given all entries and removes its own)
 *     3  an id outside [0, container_size)
 *     4  removed, but the full queue did not take the slot
 * By box (PSAMD_REMOVE_BOX): the candidates are the live owned particles with lo.x <= x < hi.x, and likewise y and z
 * (fp32 comparisons: a coordinate that is not a number is not inside), or with PSAMD_REMOVE_OUTSIDE those that are
 * not inside, in ascending global slot id: what by id does when given the ids of a psamd_export_live filtered by the
 * same predicate.  ids, count_dev and outcome_dev must be NULL and max_count 0; the launches cover every owned slot.
 * In a world larger than 1 the ranks' results add, and the union of the ranks' states is the state of one context
 * given the same call.
 *
 * Everything is enqueued on the context's stream (psamd_get_stream): nothing waits and nothing is read back.  Scratch
 * for the entries is allocated when max_count exceeds what an earlier call allocated for (that growth may wait for the
 * device); steady use neither allocates nor waits.  Like psamd_inject, the call ends a frame in progress
 * (psamd_calc_forces refuses with PSAMD_ERR_STATE until psamd_build_grid runs again) and is refused while the context's
 * stream is being captured (PSAMD_ERR_STATE: a replayed graph would bypass that bookkeeping).  The host's bound of the
 * live count stays as it is: it is an upper bound.  The call returns PSAMD_OK once the work is enqueued; only the
 * result record reports what happened.
 *
 * Cost on an MI355X at N = 2^20 (profiles/remove_cost.txt): 61 us by id for 65 536 live ids, 45 us by box
 * for as many; the host route (download_particles, download_queues, edit, two uploads) takes 156 ms there, 41 ms of it
 * in the four transfers.
 *
 * PSAMD_ERR_INVALID_ARG: a NULL context or spec, unknown flag bits, OUTSIDE without BOX, reserved != 0, max_count
 * outside [0, 2^31), by id ids NULL with max_count > 0, ids or outcome_dev not 4-byte aligned, count_dev or result_dev
 * not 8-byte aligned, by box any of ids / count_dev / outcome_dev set or max_count != 0.  PSAMD_ERR_STATE: the context
 * is wedged, or its stream is being captured.  By id with max_count == 0 the call writes a zero result and launches
 * nothing else.
 *
 * psamd_remove_result_get: the last remove's record, into host memory; waits for the context's stream. */
int psamd_remove(psamd_ctx *ctx, const psamd_remove_spec *spec);
int psamd_remove_result_get(psamd_ctx *ctx, psamd_remove_result *out);

/* ---- changing particles in place ---------------------------------------------- */
/* psamd_update: new words for particles that stay where they are -- velocity (set, or added: a kick), age, mass,
 * fertility age -- at the point of the stream where the call is made.  It is what hands a caller's own force to the
 * particles without leaving the device: psamd_probe (or an external potential, a thermostat, a push from a UI) gives the
 * caller a field, the caller forms dv, PSAMD_UPDATE_VEL | PSAMD_UPDATE_ADD applies it.  Positions are not served: a
 * particle that changes its cell is a psamd_remove plus a psamd_inject.  Not in the reference; a context that is never
 * updated computes what it always did.
 *
 * What is written.  Only the words the fields name, with the k-th entry's values: PSAMD_UPDATE_VEL vx, vy, vz = vel4[k].xyz;
 * PSAMD_UPDATE_AGE age = vel4[k].w; PSAMD_UPDATE_MASS w = w[k]; PSAMD_UPDATE_FERT fertility age = fert_age[k].  Every other
 * word of the slot keeps its bits (x, y, z beside w; ax, ay, az beside the fertility age; cell, flags), and so does every
 * other slot.  Values are written as given, bit for bit: NaNs with their payloads, infinities, -0, denormals.  With
 * PSAMD_UPDATE_ADD (a modifier of VEL; without VEL it is PSAMD_ERR_INVALID_ARG) each velocity component becomes
 * RN(v + vel4[k].c): one fp32 addition, no fused operation, no clamp -- the next step's MAX_V clamp acts as it always does.
 * Only the arrays the fields name are read, and of the context's arrays only those are written: SET stores without
 * loading, a kick loads and stores vel4.  T_DATA mirror rows, the queues and their QUEUE_INFO records, the counters and the
 * host's bound of the live count are not touched.  The caller's arrays must not lie inside the context's own
 * (psamd_device_view_get).
 *
 * By id (without PSAMD_UPDATE_EXPORT_ORDER): the entries [0, n) of `ids` are examined in entry order.  Every entry gets
 * an outcome, written to outcome_dev if given (entries at or past n are not touched):
 *     0  updated
 *     1  the slot is not live (0 <= cell < num_cells, what psamd_live_count counts)
 *     2  a valid id whose slot this context does not own
 *     3  an id outside [0, container_size)
 *     4  a later occurrence of an id this call has already updated: nothing is written for it -- THE FIRST OCCURRENCE
 *        WINS, whatever the fields (also with ADD: a particle is kicked once per call)
 * This is psamd_remove's claim rule on psamd_remove's claim words; a call leaves them as it found them, so updates and
 * removes follow one another in any order.
 *
 * By export order (PSAMD_UPDATE_EXPORT_ORDER; ids must be NULL): entry k belongs to the k-th live owned particle in
 * ascending global slot id -- the pairing of psamd_export_live's arrays, of psamd_potential's phi[] and so of a
 * psamd_probe on an export's pos4.  Entries at or past the live count get outcome 1 and count in `not_live`; live
 * particles past n are left alone; foreign, invalid and duplicate are 0.  The caller keeps the live set unchanged between
 * the export and the update (no step, inject, remove, upload or restore in between).  This is the streaming form: the
 * launches cover every owned slot, the entries are read and the slots written in contiguous runs.
 *
 * The frame.  The snapshot psamd_build_grid leaves holds x, y, z, w_eff and age; it holds no velocity and no fertility
 * age, and the pair stage reads neither.  So a call whose fields are within VEL | FERT (with or without ADD) leaves the
 * frame as it is: it keeps no host bookkeeping, allocates nothing in steady use, may be captured into a graph, and is
 * valid at every point but one (below).  Placed between psamd_calc_forces_pairs and psamd_calc_forces_apply (or
 * psamd_slab_pairs and psamd_slab_apply) the velocity it leaves is the one this step integrates, and the step's bytes are
 * those of the same update made before psamd_build_grid.  A call with MASS or AGE ends a frame in progress exactly as
 * psamd_remove does: psamd_calc_forces then refuses with PSAMD_ERR_STATE until psamd_build_grid has run again, and such a
 * call is refused while the context's stream is being captured (PSAMD_ERR_STATE).  Between psamd_slab_apply and
 * psamd_slab_finish every form returns PSAMD_ERR_STATE and the context stays usable: the departing particles are staged
 * there, and an update of the slot they leave would be lost.  psamd_step cannot be interposed, as for the other services.
 *
 * Slabs (world > 1).  By id every rank is given all entries and updates its own slots: exactly one rank answers 0 for a
 * live id, the others 2; the ranks' results add; the union of the ranks' states is the state of one context given the same
 * call.  By export order a rank's entries are its own export's.
 *
 * Everything is enqueued on the context's stream (psamd_get_stream): nothing waits and nothing is read back.  By id, scratch
 * per entry grows only when max_count exceeds every earlier psamd_update's -- that growth may wait for the device, and while
 * the stream is being captured it is refused with PSAMD_ERR_STATE; by export order there is none.  A graph that holds a
 * captured update by id is void once a later psamd_update by id has grown that scratch (the graph holds the old address):
 * make the largest call first, or capture again.  No other service touches it.
 * *result_dev and the context's own record are written by the time the stream reaches the end of the call.  The call returns
 * PSAMD_OK once the work is enqueued; only the result record reports what happened.
 *
 * Cost on an MI355X at N = 2^20 (profiles/update_cost.txt; host clock around the call plus psamd_synchronize), a kick
 * (VEL | ADD): 52 us by id for 65 536 live ids, 47 us by export order for all 321 670 live particles, beside 60 us of
 * psamd_export_live of VEL on the same context; the host route (download_particles, the addition in numpy,
 * upload_particles) takes 27.0 ms there.
 *
 * PSAMD_ERR_INVALID_ARG: a NULL context or spec, no field bit, an unknown bit, ADD without VEL, reserved != 0, max_count
 * outside [0, 2^31), by id ids NULL with max_count > 0, by export order ids not NULL, an array the fields name NULL with
 * max_count > 0, vel4 not 16-byte aligned, ids / w / fert_age / outcome_dev not 4-byte aligned, count_dev or result_dev not
 * 8-byte aligned.  PSAMD_ERR_STATE: the context is wedged, the call falls between psamd_slab_apply and psamd_slab_finish, or
 * the stream is being captured and the call has MASS or AGE or needs its scratch to grow.  max_count == 0 writes a zero
 * result and launches nothing else.
 *
 * psamd_update_result_get: the last update's record, into host memory; waits for the context's stream. */
int psamd_update(psamd_ctx *ctx, const psamd_update_spec *spec);
int psamd_update_result_get(psamd_ctx *ctx, psamd_update_result *out);

/* ---- energy ------------------------------------------------------------------ */
/* The potential of every particle in the frame's cell lists, and the potential energy, formed on the device from what
 * psamd_build_grid left (cell_start, sorted_id, the snap_soa planes).  Not in the reference: like drag, repulsion, Euler
 * and all-pairs it changes nothing in the step's arithmetic.  For every entry i of the sorted order of the own cells
 *     phi_i = - s * sum over j != i of  w_eff_j / sqrt(|x_j - x_i|^2 + eps2),     s = force_sign (0 reads as +1)
 * over exactly the bodies the force pass walks for i's cell: the 27-cell non-periodic stencil in the reference's order,
 * of each cell its first min(count, MAX_PARTICLES_PER_CELL) bodies; with PSAMD_FLAG_ALL_PAIRS every other cell of the box
 * behind them, in global index order.  A kid has w_eff = 0: it adds nothing to anybody and is given the potential at
 * its own position.  j is left out BY SORTED INDEX, not by distance: two particles at one point see each other at
 * -w / sqrt(eps2).  w_eff in these formulas is the unsigned mass (w, or 0 for a kid): the sign s appears in phi alone,
 * so repulsion flips phi and U together.  U = 1/2 * sum_i w_eff_i * phi_i in fp64; a particle whose phi is not finite (its own position, or
 * that of a body of its stencil, is not a number) counts in `nonfinite` and in no sum.
 *
 * Arithmetic: the differences and r.r in fp32 as the force pass forms them, the hardware reciprocal square root, the
 * terms added in list order in fp32 chains of at most 64 that start with every cell and are carried on in fp64.  The
 * association depends on the cell order and the lists' lengths alone: phi and U are the same bits from run to run, with
 * graphs on or off, and phi_i is the same on one context and on the slab that holds particle i.  Against an fp64 direct
 * sum phi and U stay within 1e-5 relative (tests/test_gpu_potential.py; measured: 1.5e-7 and 1e-8).
 *
 * psamd_potential: enqueued on the context's stream (psamd_get_stream) and nothing else -- it allocates nothing, waits
 * for nothing and reads nothing back (its scratch is the context's, sized at creation), so it may be captured into a
 * graph.  phi[k] belongs to the k-th live particle in ascending global slot id, the first min(count, capacity) of them:
 * entry for entry the arrays of a psamd_export_live made at the same point of the stream.  A live particle that is in no
 * list of the frame gets a quiet NaN there and does not count in `listed`.  *result_dev and the context's own record
 * (psamd_potential_result_get) are written by the time the stream reaches the end of the call.
 *
 * Valid while a frame is built and its particles have not moved: world == 1 from psamd_build_grid until the frame ends
 * (before or after psamd_calc_forces_pairs: the pair stage does not disturb what the pass reads); world > 1 from
 * psamd_slab_pairs, which unpacks the halos, until psamd_slab_apply.  Elsewhere PSAMD_ERR_STATE, also for a wedged
 * context.  psamd_step cannot be interposed: use the stage calls.
 *
 * A slab forms phi for the particles of its own state layers from its own snapshot and the received halos (all-pairs:
 * the gathered snapshot), and only if its plan lends nothing -- lentin and lentout empty, which holds for group-aligned
 * cuts; else PSAMD_ERR_UNSUPPORTED (the context stays usable): shipping phi of lent layers home would need a message of
 * its own.  The ranks' results combine like psamd_live_stats: counts and U add, the extrema take min and max.
 *
 * Far-monopole contexts (PSAMD_FLAG_FAR_MONOPOLE, PSAMD_FLAG_FAR_PYRAMID; world == 1: with PSAMD_FLAG_FAR_SLAB and world > 1 every
 * form of the call is PSAMD_ERR_UNSUPPORTED, see "far field on slabs").  Without PSAMD_POTENTIAL_FAR
 * psamd_potential and psamd_download_potential return PSAMD_ERR_UNSUPPORTED: a stencil-only phi is not the potential of
 * the field these contexts apply.  With PSAMD_POTENTIAL_FAR (host form: psamd_download_potential_far) a particle in cell c
 * sees the stencil lists of c exactly as above and, behind them, the far bodies the force pass of this context enters for
 * c, each as one body (X, Y, Z, M) of the moments: with PSAMD_FLAG_FAR_MONOPOLE every cell outside c's stencil, with
 * PSAMD_FLAG_FAR_PYRAMID the interaction set of "a pyramid of monopoles" below, levels L down to 0.  A body with M == 0 or
 * outside the set contributes no term.  The call forms the moments itself from the frame's snapshot with the pair stage's
 * own kernels -- the same bits in the same buffers -- because this window opens before the pair stage has run; the window
 * of psamd_download_cell_moments / psamd_download_level_moments is unchanged.  A far body's term is a listed body's: fp32
 * differences, unfused r.r, + eps2, the hardware reciprocal square root, one multiply by M (the same on FAST_MATH
 * contexts).  Association: within a level the cells go in level index order by blocks of 64 consecutive indices (the flat
 * method is one level; the last block may be ragged); the terms of a block's members are ONE fp32 chain in index order
 * started at +0, whose sum is carried into the fp64 accumulator; blocks in block order, levels top down, all behind the
 * stencil's chains: stencil, level L, ..., level 0.  There is no 16-part split for the potential, so a pyramid context with
 * G <= 4 gives the flat context's phi bit for bit, and a cloud inside a 2x2x2 block of cells gives the cutoff context's phi,
 * U and record byte for byte.  A kid gets the field at its own position over its cell's set.  A cell whose moments are not
 * numbers makes phi non-finite for those who take it (they count in `nonfinite`), as it does their force.  phi = (float)(-sum);
 * U, the extrema and the counts as above.  The call still allocates nothing, waits for nothing, reads nothing back and may
 * be captured; it disturbs neither the force records nor the step.  With at most one adult per cell the monopoles are exact
 * and phi is the all-pairs phi up to association.
 * Accuracy of the far phi (an fp64 model of the method against an fp64 direct sum over all bodies, 8192 bodies, uniform and
 * clustered, on 8^3 and 10^3 cells; tests/test_far_potential_cpu.py): the median particle's far phi is off by
 * 0.009-0.011 % flat and 0.02-0.11 % as a pyramid, the worst of 400 sampled by 0.04-0.07 % and 0.11-0.52 %; the stencil-only phi
 * leaves out 78-91 % for the median particle.
 * The device follows the model to 1e-5 relative (tests/test_gpu_far_potential.py).
 * Cost on an MI355X at N = 2^20 on 16^3 cells (profiles/far_potential_cost.txt): on one built frame, host clock around the call
 * + psamd_synchronize with the stream idle before it: 3.90 ms flat and 2.66 ms as a pyramid, beside 2.35 ms of psamd_potential
 * on a cutoff context of the same cloud and 3.78, 3.57 and 1.97 ms of the three contexts' pair stage.  The flat form walks 4069 far
 * bodies a (cell, slice) wave behind 27 lists of 256: 1.7 times the cutoff potential, nowhere near an all-pairs potential.
 *
 * Quadrupole contexts (PSAMD_FLAG_FAR_QUADRUPOLE; they are pyramid contexts).  PSAMD_POTENTIAL_FAR alone promises each far body
 * as one body (X, Y, Z, M), which is not the field such a context applies: without a bit and with PSAMD_POTENTIAL_FAR alone
 * psamd_potential, psamd_download_potential and psamd_download_potential_far return PSAMD_ERR_UNSUPPORTED (the context stays
 * usable).  With PSAMD_POTENTIAL_FAR | PSAMD_POTENTIAL_QUADRUPOLE (host form: psamd_download_potential_flags) every member of the
 * interaction set adds, beside its monopole term, the quadrupole term of "quadrupoles on the pyramid" below -- in the
 * convention of these sums (sum of w u, phi = (float)(-sum)) t_q = 1.5 (d.C.d) u^5 - 0.5 T u^3, the term whose gradient is that
 * section's a_q -- from the ten planes the call forms itself.  Association: the stencil's chains and every block's monopole
 * chain are PSAMD_POTENTIAL_FAR's on a pyramid context, bit for bit; behind a block's monopole chain comes that block's
 * quadrupole chain -- ONE fp32 chain from +0, in index order, over the members of the monopole chain -- and each of the two is
 * carried into the fp64 accumulator by an addition of its own (acc += monopole chain; acc += quadrupole chain); blocks in
 * block order, levels top down.  Consequences: with every C an exact zero (G <= 4, at most one adult a cell, kids anywhere)
 * every quadrupole chain is +0, and phi, U and the record are those a PSAMD_FLAG_FAR_PYRAMID context returns under
 * PSAMD_POTENTIAL_FAR, byte for byte; a cloud inside a 2x2x2 block of cells gives the cutoff context's phi, U and record byte
 * for byte.  Window, PSAMD_ERR_STATE, alignment, capacity and "allocates nothing, waits for nothing, may be captured" are
 * unchanged.
 * Accuracy of the quadrupole far phi (the fp64 model against an fp64 direct sum, the clouds above;
 * tests/test_far_quad_potential_cpu.py): the median particle's phi is off by 0.006-0.011 %, the worst of 400 sampled by
 * 0.029-0.042 %, where the pyramid of monopoles is off by 0.02-0.11 % and 0.11-0.52 %: the median falls to 0.06-0.41 of the
 * pyramid's.  The device follows the model to 1e-5 relative (tests/test_gpu_far_quad_potential.py).
 * Cost on an MI355X at N = 2^20 on 16^3 cells (profiles/far_quad_potential_cost.txt; the far potential's protocol, both contexts in
 * one run): 3.59 ms on the quadrupole context beside 2.67 ms of the far potential on a pyramid context, 1.35 times.
 *
 * PSAMD_ERR_INVALID_ARG: a NULL context or spec, flags with an unknown bit (PSAMD_POTENTIAL_FAR is one on a context with
 * neither far flag, PSAMD_POTENTIAL_QUADRUPOLE on a context without PSAMD_FLAG_FAR_QUADRUPOLE), PSAMD_POTENTIAL_QUADRUPOLE without
 * PSAMD_POTENTIAL_FAR, or reserved not 0, capacity < 0, phi not 4-byte aligned, phi NULL with capacity > 0, result_dev not
 * 8-byte aligned.
 *
 * psamd_potential_result_get: the last call's record, into host memory; waits for the context's stream.
 * psamd_download_potential: the same pass into host memory (phi: `capacity` floats or NULL with capacity 0; out may be
 * NULL); only the min(count, capacity) entries cross PCIe and are written, count being the live count that
 * psamd_download_live reports at the same point (with no fields and capacity 0 it costs two small launches).  Waits for
 * the context's stream.
 * psamd_download_potential_far: the host form of a PSAMD_POTENTIAL_FAR call, otherwise psamd_download_potential; on a
 * context with neither far flag PSAMD_ERR_UNSUPPORTED.
 * psamd_download_potential_flags: the host form of a psamd_potential call with these spec flags, the same body as the two
 * above; `flags` is validated as psamd_potential validates it, ahead of the other arguments (so PSAMD_POTENTIAL_FAR on a
 * context with neither far flag is PSAMD_ERR_INVALID_ARG here).  The host form of every later bit: no further _xxx form will
 * be added. */
int psamd_potential(psamd_ctx *ctx, const psamd_potential_spec *spec);
int psamd_potential_result_get(psamd_ctx *ctx, psamd_potential_result *out);
int psamd_download_potential(psamd_ctx *ctx, float *phi, int64_t capacity, psamd_potential_result *out);
int psamd_download_potential_far(psamd_ctx *ctx, float *phi, int64_t capacity, psamd_potential_result *out);
int psamd_download_potential_flags(psamd_ctx *ctx, uint32_t flags, float *phi, int64_t capacity, psamd_potential_result *out);

/* ---- the field at chosen points ------------------------------------------------ */
/* psamd_probe: the acceleration and the potential of the frame's field at points of the caller's choosing -- under a
 * cursor, on the nodes of a grid, along a field line, at massless tracers the caller integrates itself.  A probe is no
 * particle: it has a position and nothing else, it enters no list and no life cycle.  Not in the reference; the step's
 * arithmetic is untouched.
 *
 * Outcomes.  Every entry k < n has a cell by the rule psamd_inject uses (Geometry::locate, the fp64 floor test):
 *     0  served
 *     1  outside the box; coordinates that are not numbers, and huge ones, count as outside
 *     2  a valid cell that is not one of this context's compute cells -- the cells its force pass walks, lent-in layers
 *        included (world > 1 only: exactly one rank serves each in-box probe, on any plan)
 * An entry with outcome 1 or 2 gets the quiet NaN 0x7fc00000 in all four words of out4[k]; a served entry gets 0.0f in
 * the components that were not asked for.  Entries at or past n are not touched.
 *
 * Bodies.  A served probe at x sees exactly the bodies the force pass walks for its cell: the 27-cell non-periodic
 * stencil in the reference's order, of each cell the first min(count, MAX_PARTICLES_PER_CELL) entries of the sorted
 * snapshot with their w_eff.  A kid has w_eff = 0 and the origin as its snapshot position; force_sign is folded into
 * w_eff.  Nothing is left out: a probe has no own entry.
 *
 * Acceleration.  One fp32 chain per component starts at +0 and every body is added in that order by the context's own
 * pair form -- the exact forms of the force pass, or the fast ones on a PSAMD_FLAG_FAST_MATH context.  Consequence: on an
 * exact-path cutoff context (a softening length in the lean range, which the default is) a probe at the position of an
 * adult that the frame's force pass serves returns that particle's (ax, ay, az) BIT FOR BIT -- the particle's own term is
 * r * s with r = 0, which adds a zero.  A softening length outside the lean range takes the generic exact form, which
 * skips massless bodies and has no such promise for a probe on a particle (1/sqrt(eps2^3) need not be finite there).
 *
 * Potential.  psamd_potential's arithmetic and association, unchanged: fp32 chains of at most 64 that start with every
 * cell and are carried on in fp64, phi = (float)(-sum).  Consequence: a probe at the true position of a listed kid (its
 * pos4, not its snapshot entry) returns that kid's phi from psamd_potential bit for bit.  A probe on an adult returns
 * that adult's phi plus its own term, -s * w / sqrt(eps2) up to rounding: psamd_potential leaves the own entry out, a
 * probe has none to leave out.
 *
 * All-pairs contexts (PSAMD_FLAG_ALL_PAIRS), world == 1: every other cell of the box follows the stencil in global index
 * order, psamd_potential's walk.  phi keeps the association above.  For the acceleration each far cell's terms go into
 * fp32 chains per component that start at +0 with the cell, hold at most 64 terms and are carried on in fp64, and
 * a = (float)((double)a_stencil + far).  This is NOT the force pass's far-field association (16 partial sums per
 * particle): equality with the force record is promised for cutoff contexts only.  With empty far cells the result is
 * the cutoff result bit for bit.  With world > 1 the call returns PSAMD_ERR_UNSUPPORTED; the context stays usable.
 *
 * Far-monopole contexts (PSAMD_FLAG_FAR_MONOPOLE, PSAMD_FLAG_FAR_PYRAMID; world == 1: with PSAMD_FLAG_FAR_SLAB and world > 1 the
 * call is PSAMD_ERR_UNSUPPORTED, see "far field on slabs").  Without PSAMD_PROBE_FAR the call
 * returns PSAMD_ERR_UNSUPPORTED.  With it (beside ACC and / or PHI; alone it is PSAMD_ERR_INVALID_ARG) a served probe in cell
 * c sees the stencil of c as above and then the far bodies the force pass enters for c, from moments the call forms itself
 * (psamd_potential's far form, "energy" above).  phi: that far form's terms and association.  Acceleration: the force
 * pass's association exactly -- every far body through the context's own pair form, chains per block of 64 from +0; flat:
 * the block sums into the 16 parts by PSAMD_FLAG_FAR_MONOPOLE's rule, a = (((stencil + part 0) + ...) + part 15); pyramid: a
 * level's sum is its block chains added in block order to +0, a = ((stencil + level L) + ...) + level 0.  Consequence: on an
 * exact-path far context a PSAMD_PROBE_ACC | PSAMD_PROBE_FAR probe at the position of an adult the force pass serves returns
 * that particle's force record BIT FOR BIT; a PHI probe at a listed kid's true position returns that kid's far phi bit for
 * bit.  Outcomes, the NaN words, the determinism promise and count_dev are unchanged.
 *
 * Quadrupole contexts (PSAMD_FLAG_FAR_QUADRUPOLE).  Without a modifier and with PSAMD_PROBE_FAR alone the call returns
 * PSAMD_ERR_UNSUPPORTED (monopoles only are not that context's field).  With PSAMD_PROBE_FAR | PSAMD_PROBE_QUADRUPOLE beside ACC
 * and / or PHI every far body adds its quadrupole term too.  phi: psamd_potential's quadrupole form ("energy" above), terms and
 * association.  Acceleration: the force pass's association exactly -- per block the monopole chain and, behind each group's
 * pair terms, the block's quadrupole chain from +0; per level the monopole sum and the quadrupole sum add up in block order to
 * +0, the level's part is RN(monopole sum + quadrupole sum), and a = ((stencil + part L) + ...) + part 0.  Consequences: on an
 * exact or PSAMD_FLAG_FAST_MATH quadrupole context an ACC | FAR | QUADRUPOLE probe at the position of an adult the force pass
 * serves returns that adult's force record BIT FOR BIT; a PHI | FAR | QUADRUPOLE probe at a listed kid's true position returns
 * that kid's phi from psamd_potential (FAR | QUADRUPOLE) bit for bit; with every C an exact zero the words are those a
 * PSAMD_FLAG_FAR_PYRAMID context returns under PSAMD_PROBE_FAR, and for a cloud inside a 2x2x2 block of cells the cutoff
 * context's, byte for byte.  A probe's words depend on its position and the frame alone, also on whether ACC and PHI are asked
 * for together or one by one.
 * Cost (profiles/far_quad_potential_cost.txt): 65 536 probes, ACC | PHI, at N = 2^20, beside far probes on a pyramid context in
 * the same run: on particles' own positions 6.13 ms beside 5.37 ms (1.14 times), on a regular grid 3.62 ms beside 3.21 ms
 * (1.13 times).
 *
 * Cost (profiles/far_potential_cost.txt): 65 536 far probes, ACC | PHI, at N = 2^20 (same protocol as the far potential): on
 * particles' own positions 7.96 ms flat and 5.46 ms as a pyramid beside 4.69 ms of plain probes on a cutoff context; on a regular
 * grid 4.66 and 3.24 ms beside 2.76 ms.
 *
 * Determinism.  A probe's four words depend on its position and the frame alone: not on the other probes, their order,
 * max_count, graphs, or whether a slab or one context serves it.
 *
 * Valid in psamd_potential's window: world == 1 from psamd_build_grid until the frame ends, world > 1 between
 * psamd_slab_pairs and psamd_slab_apply; elsewhere PSAMD_ERR_STATE, also for a wedged context.  psamd_potential's
 * refusal of plans that lend layers does not apply: a rank serves the probes of the cells it computes.
 *
 * Everything is enqueued on the context's stream (psamd_get_stream): nothing waits, nothing is read back, the call ends
 * no frame and keeps no host bookkeeping.  Scratch per entry grows only when max_count exceeds every earlier call's
 * (that growth may wait for the device); so the call may be captured into a graph whenever no growth is needed, and
 * returns PSAMD_ERR_STATE if growth is needed while the stream is being captured.  *result_dev and the context's own
 * record (psamd_probe_result_get) are written by the time the stream reaches the end of the call.
 *
 * Cost on an MI355X at N = 2^20 (profiles/probe_cost.txt), ACC | PHI: 1.12 ms for 65 536 probes on particles' own
 * positions, 0.89 ms for as many on a regular grid, beside 0.48 ms of psamd_potential and 0.39 ms of the force pass on
 * the same frames.  The cost follows the (wave, distinct cell) walks: 16 probes to a cell use a quarter of the lanes.
 *
 * PSAMD_ERR_INVALID_ARG: a NULL context or spec, fields without ACC and PHI or with unknown bits (PSAMD_PROBE_FAR is one
 * on a context with neither far flag, PSAMD_PROBE_QUADRUPOLE on a context without PSAMD_FLAG_FAR_QUADRUPOLE),
 * PSAMD_PROBE_QUADRUPOLE without PSAMD_PROBE_FAR, reserved != 0, max_count outside
 * [0, 2^31), pos4 or out4 NULL with max_count > 0 or not 16-byte aligned, outcome_dev not 4-byte aligned, count_dev or
 * result_dev not 8-byte aligned.  max_count == 0 writes a zero result and launches nothing else.
 *
 * psamd_probe_result_get: the last probe's record, into host memory; waits for the context's stream. */
int psamd_probe(psamd_ctx *ctx, const psamd_probe_spec *spec);
int psamd_probe_result_get(psamd_ctx *ctx, psamd_probe_result *out);

/* ---- mass on a lattice ---------------------------------------------------------- */
/* psamd_deposit: the source of the field psamd_probe serves, as a field -- the mass density of the frame on a regular
 * lattice, cloud-in-cell, for a volume renderer, a clump or void analysis, a particle-mesh solver of the caller's, or
 * Poisson's equation checked against psamd_probe's phi on the same nodes.  The bodies are sorted by cell, so every voxel
 * is GATHERED from the 27-cell stencil of its cell in a fixed order: no floating-point atomic, the same bytes from run to
 * run and with graphs on or off, and on slabs every voxel formed entirely on one rank.  Not in the reference; the step's
 * arithmetic is untouched, no force record, particle or queue is written, and PSAMD_ABI_VERSION stays 8.
 *
 * Lattice.  refine = k in {1, 2, 4} voxels per cell edge: M = G k voxels per axis (G = grid_dim), h = cell_size / k.  The
 * axes are the cell axes of the locate rule, (q1, q2, q3) = (-y, x, -z).  Voxel (n1, n2, n3) has index (n3 M + n1) M + n2 --
 * the cell index's order; as a [M][M][M] array it is indexed [n3][n1][n2] -- its centre lies at q_a = (n_a + 1/2 - (G / 2) k) h
 * with G / 2 the integer division of the cell rule, and it belongs to cell (n_a div k).
 *
 * Bodies.  Those the force pass walks: of every cell the first min(count, MAX_PARTICLES_PER_CELL) entries of the sorted
 * snapshot (x, y, z, w_eff), with mass m = |w_eff|: force_sign does not enter, as in psamd_potential's U.  A kid has
 * w_eff = 0 and adds nothing, as it adds nothing to the force: the volume is the density of GRAVITATING mass, not of all
 * live particles.  A body with any of x, y, z, w_eff not finite adds nothing and counts in `skipped`, once, by its own cell.
 *
 * Weights.  All in fp32, every operation rounded on its own, nothing fused.  Per axis, with s the signed coordinate (-y, x,
 * -z: exact), inv_h = (float)((double)k / cell_size) and off = (float)((G / 2) k) - 0.5f (exact):
 *     t = RN(s inv_h);  u = RN(t + off);  u_c = min(max(u, 0), M - 1);  n0 = (int)floor(u_c);  f = u_c - n0  (exact)
 * and the body gives the weight RN(1 - f) to voxel n0 and f to n0 + 1 of that axis; a weight for n0 + 1 == M is zero and
 * dropped.  The clamp folds mass beyond the outermost voxel centres onto the face voxels: the deposit conserves mass and is
 * not periodic (nor is the stencil).  A body's term for a voxel is RN(RN(RN(W1 W2) W3) m).
 *
 * Stencil rule.  A body of cell c contributes only to voxels whose cell lies within one cell of c on every axis.  That is
 * always so for particles the step itself places (the margin is at least 1/8 cell against a few ulp); it is stated because
 * uploaded records may carry a cell that does not fit their position, and it is what makes the gather over the 27-cell
 * stencil complete.  A voxel is decided by u alone (n0 and n0 + 1), never by re-deriving the body's cell.
 *
 * Sum.  A voxel's value is (float) of the fp64 sum of its terms.  Association: one wave forms the voxel; lane l of its 64
 * takes entries l, l + 64, l + 128 ... of every list and adds its terms from +0 in fp64 -- the stencil's cells in the
 * reference's order (the cell itself first), a cell's entries in list order -- and the 64 lane sums close in a butterfly: every
 * lane adds the sum of lane l ^ 32, then of l ^ 16, ^ 8, ^ 4, ^ 2, ^ 1.  The order depends on the voxel and on the lists'
 * lengths alone: not on the launch, the rank or the plan.  A voxel nobody reaches is +0.0f.  Against the same terms summed
 * in any other order only the last rounding can differ: 1 ulp.
 *
 * Result.  voxels: those this context wrote, its compute cells times k^3; bodies / skipped: the listed bodies of those cells
 * that are finite / are not; mass: the fp64 sum of this context's voxel sums before their rounding to float -- per task (a
 * cell's block of at most 2 x 2 x 2 voxels: 1, 1, 8 tasks a cell for k = 1, 2, 4; the blocks by (n3, n1, n2), the cells in the
 * force pass's order) the voxels in (n3, n1, n2) order, four tasks at a time, those partials in one serial chain; vmax: the
 * largest float written as a double, -inf if none.  The total mass equals the bodies' within 2^-21 relative (four roundings
 * of a term).
 *
 * Slabs.  A rank writes the voxels of its compute cells -- psamd_probe's rule, lent-in layers included: exactly one rank
 * serves every voxel on any plan, group-aligned or not -- at their index in the FULL lattice and leaves every other entry of
 * `out` alone.  The union of the ranks' writes is one context's array bit for bit; voxels, bodies, skipped and mass add over
 * the ranks, vmax takes the maximum.  Every context kind is served alike -- cutoff, PSAMD_FLAG_FAST_MATH, all-pairs, the three
 * far methods and far slabs (PSAMD_FLAG_FAR_SLAB): the quantity depends on the lists alone.
 *
 * Valid in psamd_potential's window: world == 1 from psamd_build_grid until the frame ends, world > 1 between
 * psamd_slab_pairs and psamd_slab_apply; elsewhere PSAMD_ERR_STATE, also for a wedged context.  The call neither ends nor
 * disturbs the frame, the force records or the step.
 *
 * Everything is enqueued on the context's stream (psamd_get_stream): nothing waits, nothing is read back, no host
 * bookkeeping; PSAMD_OK says the work is enqueued, only the result record says what happened.  The scratch (48 bytes per
 * compute cell: the partials of mass, vmax and the counts) is allocated at psamd_create, so the call allocates nothing and
 * may always be captured into a graph.  *result_dev and the context's own record (psamd_deposit_result_get) are written by
 * the time the stream reaches the end of the call.
 *
 * psamd_download_deposit: the same pass into host memory -- staged on the device, the stream waited for, the WHOLE lattice
 * copied (capacity >= M^3 floats).  On a slab the entries of voxels the rank does not serve are +0, so the ranks' arrays
 * add up to one context's exactly (every voxel has one non-zero contributor).  `result` may be NULL.
 *
 * Cost on an MI355X at N = 2^20 on 16^3 cells (scripts/deposit_cost.py; profiles/deposit_cost.txt), measured: 0.066 ms at refine 1
 * (4 096 voxels), 0.078 ms at refine 2 (32 768), 0.33 ms at refine 4 (262 144), beside 0.51 ms of psamd_potential on the same frame
 * in the same run (host clock around the call plus psamd_synchronize, the stream idle before it).  At refine 4 a cell's eight
 * blocks each walk the cell's 27 lists.
 *
 * PSAMD_ERR_INVALID_ARG: a NULL context or spec, flags != 0, refine not 1, 2 or 4, out NULL or not 4-byte aligned,
 * capacity < M^3, result_dev not 8-byte aligned.
 *
 * psamd_deposit_result_get: the last deposit's record, into host memory; waits for the context's stream. */
int psamd_deposit(psamd_ctx *ctx, const psamd_deposit_spec *spec);
int psamd_deposit_result_get(psamd_ctx *ctx, psamd_deposit_result *out);
int psamd_download_deposit(psamd_ctx *ctx, int32_t refine, float *out, int64_t capacity, psamd_deposit_result *result);

/* ---- a lattice field at the particles ---------------------------------------------- */
/* psamd_sample: a field the CALLER holds on psamd_deposit's lattice -- a potential or a force solved from the deposit with an
 * FFT or a stencil, a hand-made external field -- read back at points of the caller's choosing or at the live particles
 * themselves, cloud-in-cell.  It is the exact adjoint of psamd_deposit: the weight a body gives a voxel there is the weight
 * that voxel's value has in the body's sample here, the same fp32 number.  Adjoint weights are what make a particle-mesh
 * force free of self-force and momentum-conserving; with psamd_update (VEL | ADD | EXPORT_ORDER) behind it the loop
 * deposit -> solve -> sample -> kick stays on the device.  psamd_probe serves the library's own pair field; this serves the
 * caller's.  Not in the reference; the step's arithmetic is untouched and PSAMD_ABI_VERSION stays 8.
 *
 * Lattice and axes.  psamd_deposit's, word for word ("mass on a lattice" above): refine = k in {1, 2, 4}, M = G k voxels per
 * axis, the axes (q1, q2, q3) = (-y, x, -z), voxel (n1, n2, n3) at index (n3 M + n1) M + n2, inv_h and off as there.  `field`
 * holds one float per voxel, or with PSAMD_SAMPLE_VEC4 one float4 (say a force and a potential, solved together); `out` has
 * the same layout per entry.
 *
 * Weights.  Per axis u = RN(RN(s inv_h) + off), u_c = min(max(u, 0), M - 1), n0 = (int)floor(u_c), f = u_c - n0 (exact); the
 * weights are RN(1 - f) for voxel n0 and f for n0 + 1.  Every operation is rounded on its own, nothing is fused.
 *
 * Terms.  The eight voxels (n3 + d3, n1 + d1, n2 + d2) are visited in the order (d3, d1, d2), each 0 then 1 -- the deposit's
 * loop order -- with W = RN(RN(W1 W2) W3).  A voxel with an axis weight of exactly 0 is NOT READ and adds no term: n0 + 1 == M
 * is never touched, and a NaN in a voxel the point does not reach is harmless.  Otherwise the term is RN(W v) in fp32, per
 * component.
 *
 * Sum.  One fp64 chain per component starts at +0 and takes the terms in that order; value = (float)sum and every word of
 * out[k] is RN(scale value).  Consequences: with scale 1 a point on a voxel centre returns that voxel's value (-0 becomes
 * +0); a point beyond the outermost centres returns the face voxel's value -- the deposit's fold, read backwards.
 *
 * Outcomes.  Every entry k < n:
 *     0  served
 *     1  outside the box by Geometry::locate (the fp64 floor test psamd_probe and psamd_inject use); coordinates that are not
 *        numbers, and huge ones, count as outside
 * An entry with outcome 1 gets the quiet NaN 0x7fc00000 in every word of out[k].  Entries at or past n are not touched.  There
 * is no "foreign" outcome: the call reads the geometry, the caller's lattice and, with PSAMD_SAMPLE_EXPORT_ORDER, the context's
 * pos4 and cell.  It reads no frame.
 *
 * Result.  done: the entries examined; served / outside: those with outcome 0 / 1; nonfinite: of the served, the entries
 * with a word of out that is not finite (the lattice's, or scale's).
 *
 * Slabs.  A rank serves every in-box point it is given, whichever rank owns the cell, and the caller hands each rank the
 * WHOLE lattice: psamd_deposit writes a rank's voxels only, so the ranks' lattices are summed first (psamd_download_deposit's
 * arrays add up exactly across ranks, see above).  By PSAMD_SAMPLE_EXPORT_ORDER a rank's entries are its own export's.  The
 * words are the single context's bytes.
 *
 * PSAMD_SAMPLE_EXPORT_ORDER.  pos4 is NULL; entry k is the k-th live owned particle in ascending slot id -- the pairing of
 * psamd_export_live, of psamd_potential's phi[] and of psamd_update's order form, so out feeds psamd_update as it is -- and
 * its x, y, z are read from the context.  Live particles past n are not served; entries at or past the live count are not
 * touched; done = min(n, live count).  A live particle whose position is not a number gets outcome 1.  Valid wherever
 * psamd_export_live is valid, except between psamd_slab_apply and psamd_slab_finish (the departing particles are staged:
 * PSAMD_ERR_STATE, as psamd_update).
 *
 * Window.  The points form is valid at any stage of any context kind -- before the first psamd_build_grid, mid-frame, on
 * far-field slabs.  The only refusal is a wedged context (PSAMD_ERR_STATE).  The call neither ends nor disturbs a frame and
 * writes nothing of the context's but its own result record.
 *
 * Everything is enqueued on the context's stream (psamd_get_stream): nothing waits, nothing is read back, no host
 * bookkeeping; PSAMD_OK says the work is enqueued, only the result record says what happened.  The scratch -- three integer
 * counters, and by export order psamd_update's live count per tile of slots -- is allocated at psamd_create, so the call
 * allocates nothing and may always be captured into a graph.  The counters meet by integer atomics, in any order the same
 * record; no floating-point atomic appears anywhere.  *result_dev and the context's own record (psamd_sample_result_get) are
 * written by the time the stream reaches the end of the call.
 *
 * Determinism.  An entry's words depend on its position, the lattice and scale alone: not on the other entries, max_count,
 * graphs, the form (points or export order) or the rank.
 *
 * Cost on an MI355X at N = 2^20 on 16^3 cells, 321 670 live in 2 997 648 owned slots (scripts/sample_cost.py;
 * profiles/sample_cost.txt), measured: by export order 0.069 ms (float) and 0.074 ms (float4) at refine 2 -- 0.068 to 0.075 ms over
 * the three refines and both layouts -- and 0.090 to 0.092 ms for the points form at the export's positions, beside 0.58 ms (float)
 * and 0.97 ms (float4) for psamd_export_live plus the same interpolation written in torch (index arithmetic, eight gathers, a
 * weighted sum) in the same run: 8 and 13 times the order form.  The export of POS alone took 0.062 ms and psamd_probe ACC | PHI
 * on the same positions 1.30 ms (host clock around the call plus psamd_synchronize, the stream idle before it).
 *
 * PSAMD_ERR_INVALID_ARG: a NULL context or spec, unknown flag bits, reserved != 0, refine not 1, 2 or 4, capacity < M^3,
 * max_count outside [0, 2^31), field NULL, out NULL with max_count > 0, pos4 NULL without PSAMD_SAMPLE_EXPORT_ORDER (with
 * max_count > 0) or not NULL with it, pos4 not 16-byte aligned, field or out not 16-byte aligned under PSAMD_SAMPLE_VEC4 or not
 * 4-byte aligned without it, outcome_dev not 4-byte aligned, count_dev or result_dev not 8-byte aligned.  max_count == 0
 * writes a zero result and launches nothing else.
 *
 * psamd_sample_result_get: the last sample's record, into host memory; waits for the context's stream. */
int psamd_sample(psamd_ctx *ctx, const psamd_sample_spec *spec);
int psamd_sample_result_get(psamd_ctx *ctx, psamd_sample_result *out);

/* ---- neighbours within a radius ---------------------------------------------------- */
/* psamd_neighbours: every pair within a radius, in CSR form, in a fixed order, lined up with psamd_export_live.  With the
 * export, torch gathers over the lists and psamd_update (VEL | ADD | EXPORT_ORDER) a caller builds a short-range force of its
 * own -- an SPH density, springs, flocking, a soft contact -- without a download and without a second grid.  Not in the
 * reference; the step's arithmetic is untouched and PSAMD_ABI_VERSION stays 8.
 *
 * Queries.  A query is a listed particle of the context's own cells: entry gi of the sorted order with
 * gi - cell_start[c] < min(count_c, MAX_PARTICLES_PER_CELL) -- exactly the set psamd_potential forms phi for.  Its position is
 * the snapshot's; a kid's snapshot position is the origin, so a kid is queried at its true position, from its slot.
 *
 * Candidates.  The bodies the force pass walks for the query's cell, in its order: the 27-cell non-periodic stencil in the
 * reference's order, the own cell first; of each cell the first min(count, MAX_PARTICLES_PER_CELL) entries in list order (ids
 * ascending).  Left out are the query's own entry -- by sorted index: two particles at one point are each other's neighbours
 * -- and every kid (its snapshot entry is not where it is, and a halo carries nothing better): a kid has neighbours and is
 * nobody's neighbour.  Over-age particles are candidates like any other.
 *
 * Test.  fp32, nothing fused: rx = xj - xi (ry, rz alike), d2 = RN(RN(RN(rx rx) + RN(ry ry)) + RN(rz rz)), r2 = RN(radius
 * radius); j is a neighbour iff d2 <= r2, and a NaN on either side is no neighbour.  d2 is symmetric bit for bit: two adults
 * inside their lists' capacities list each other or neither.
 *
 * Radius.  Finite, > 0 and (double)radius <= cell_size, else PSAMD_ERR_INVALID_ARG.  The definition is OVER THE STENCIL: with
 * radius == cell_size a pair that lies a rounding inside the radius across two cell walls is not in the stencil and is not
 * listed.  The stencil is not periodic, as the force is not: a pair across the box's wrap is not listed.
 *
 * Outputs.  All optional, in export order: entry k is the k-th live owned particle in ascending global slot id, for the first
 * m = min(live, capacity) of them -- psamd_export_live's and phi[]'s pairing.
 *     count[k]       the number of neighbours; it depends on no list capacity.  -1: a live particle that is in no list of the
 *                    frame (psamd_potential gives it a NaN)
 *     nearest[k], nearest_d2[k]   the neighbour with the smallest d2, ties to the lower global slot id; none: -1 and +inf
 *     offsets[0..m]  the exclusive prefix of max(count, 0) over the export order; offsets[m] is the entries these m have
 *     list[p]        the neighbours of entry k at offsets[k] <= p < offsets[k + 1], in walk order (stencil order, list order
 *                    inside a cell).  Position p is written iff p < list_capacity: a buffer too small cuts the tail and
 *                    nothing else.  list needs offsets (PSAMD_ERR_INVALID_ARG without)
 * A neighbour is named by its global slot id (a halo's particle by the id the halo carried).  With PSAMD_NEIGHBOURS_INDEX it is
 * named by its export index, so that pos[list] is a plain gather; a neighbour whose export index is >= capacity keeps its true
 * index.  The index form is served for world == 1 only (PSAMD_ERR_UNSUPPORTED otherwise).
 *
 * Record.  listed: the queries; pairs: the sum of all queries' counts, the whole context's (directed pairs); wanted:
 * offsets[m] -- written = min(wanted, list_capacity) is the caller's to form; max_count; d2_min over all neighbours, +inf if
 * there is none.  A slab world's records combine: the counts add, max_count and d2_min take the maximum and the minimum.
 *
 * Window and refusals: psamd_potential's.  world == 1: from psamd_build_grid until the frame ends; world > 1: between
 * psamd_slab_pairs and psamd_slab_apply, and only on a plan that lends nothing (a lending plan: PSAMD_ERR_UNSUPPORTED, the
 * context stays usable); elsewhere and on a wedged context PSAMD_ERR_STATE.  The query does not depend on the force model: it
 * is served on cutoff, all-pairs and all far-field contexts with world == 1, on cutoff and PSAMD_FLAG_FAR_SLAB contexts with
 * world > 1; an all-pairs context with world > 1 returns PSAMD_ERR_UNSUPPORTED.  The call changes nothing in the frame, the
 * force records or the step.
 *
 * Stream.  Everything is enqueued on the context's stream; nothing waits, nothing is read back.  The scratch (the count and the
 * nearest pair per sorted entry and per slot, the slot -> export index table, the slots' starts) is the context's: the first
 * call allocates it -- that call may wait for the device and returns PSAMD_ERR_STATE under a capture -- and it never grows, its
 * size depends on the container alone; every later call may be captured into a graph.  Contexts that never call pay nothing.
 *
 * Determinism.  Every output word is an integer or one fp32 value with a fixed operand order: the same bytes from run to run,
 * with graphs or without.  By id, the union of a slab world's outputs is the single context's byte for byte (offsets compared
 * as counts).
 *
 * Cost on an MI355X at N = 2^20 on 16^3 cells, 321 502 live in 2 997 648 owned slots (scripts/neighbours_cost.py;
 * profiles/neighbours_cost.txt), measured: count and offsets 0.82 ms at radius 0.4 (wanted 5 356), 0.83 ms at 1.0 (78 260) and
 * 0.83 ms at cell_size (8 712 345); with the lists 1.36, 1.35 and 1.39 ms; psamd_potential beside them 0.62 ms (a host clock
 * around the call plus psamd_synchronize, the stream idle before it).  The call does not get cheaper with the radius: it walks
 * the whole stencil whatever the radius is.
 *
 * PSAMD_ERR_INVALID_ARG: a NULL context or spec, unknown flag bits, a bad radius, capacity < 0 or list_capacity < 0, count,
 * nearest, nearest_d2 or list not 4-byte aligned, offsets or result_dev not 8-byte aligned, list without offsets.
 *
 * psamd_neighbours_result_get: the last call's record, into host memory; waits for the context's stream.
 * psamd_download_neighbours: the host form -- the same passes staged on the device, then what was asked for copied into host
 * arrays (any may be NULL) of capacity (offsets: capacity + 1) and list_capacity entries; waits for the stream. */
int psamd_neighbours(psamd_ctx *ctx, const psamd_neighbours_spec *spec);
int psamd_neighbours_result_get(psamd_ctx *ctx, psamd_neighbours_result *out);
int psamd_download_neighbours(psamd_ctx *ctx, uint32_t flags, float radius, int32_t *count, int32_t *nearest, float *nearest_d2,
                              int64_t *offsets, int64_t capacity, int32_t *list, int64_t list_capacity, psamd_neighbours_result *result);

/* ---- groups within a radius --------------------------------------------------------- */
/* psamd_groups: the friends-of-friends groups -- the connected components of psamd_neighbours' "within a radius" relation --
 * on the device, without a pair list: which particles hang together, how many groups there are and how big each one is.
 * With the export and torch.index_add_ over group[] a caller has group masses and centres, a clump finder or a halo
 * catalogue, without a download.  Not in the reference; the step's arithmetic is untouched and PSAMD_ABI_VERSION stays 8.
 *
 * Members.  The listed particles of the context's own cells that are not kids: psamd_neighbours' candidates seen as queries.
 * A kid is nobody's neighbour there, so a relation that took kids in would not be symmetric: a kid is no member.  A kid and a
 * live particle that is in no list of the frame have group[k] = -1.  Over-age particles are members like any other.  A member
 * with a non-finite coordinate links to nobody and is a group of one.
 *
 * Links.  psamd_neighbours' test, word for word: the same fp32 d2 with the same operand order, d2 <= r2 with r2 = RN(radius
 * radius), over the 27-cell non-periodic stencil, the own entry left out by sorted index -- two particles at one point are
 * linked.  d2 is symmetric bit for bit and so is the stencil: the relation is symmetric, and the walk takes each pair from
 * the side of its higher slot only.  As there, the definition is OVER THE STENCIL and the stencil is not periodic.
 *
 * Groups.  The connected components of the links over the members, numbered g = 0 .. groups - 1 in ascending order of their
 * smallest member's global slot id -- the export order is ascending slot id, so also of their smallest export index.
 *     group[k]        entry k of the export order (psamd_export_live's pairing, the first m = min(live, capacity)): its
 *                     group's number, always the true g, also when g >= group_capacity; -1: no member
 *     group_first[g]  the group's smallest member, by global slot id or, with PSAMD_GROUPS_INDEX, by export index (an index at
 *                     or past capacity is kept true)
 *     group_size[g]   its member count
 * Entry g of the two tables is written iff g < group_capacity: tables too small cut the tail and nothing else.
 *
 * Record.  members; groups, singles included; links: the undirected member pairs with d2 <= r2 over the stencil (on a frame
 * without kids twice this is psamd_neighbours' pairs); singles: the groups of one; largest: the largest group's size, 0 if
 * there is no member; unfinished: see Bounded loops.
 *
 * Window and refusals.  world == 1 only: a group can span ranks, and merging the ranks' groups across the slab cuts is a
 * later change; world > 1 returns PSAMD_ERR_UNSUPPORTED and leaves the context usable.  With world == 1 the window is
 * psamd_potential's: from psamd_build_grid until the frame ends; elsewhere and on a wedged context PSAMD_ERR_STATE.  The
 * result does not depend on the force model: the call is served on cutoff, fast-math, all-pairs and all far-field contexts
 * alike.  It writes nothing of the frame, the force records or the step.
 *
 * Stream.  psamd_neighbours' rules: everything is enqueued on the context's stream, nothing waits, nothing is read back.  The
 * scratch (six words per owned slot: the union-find, the members, the roots, the sizes, the numbers, the slot -> export index
 * table) is the context's: the first call allocates it -- that call may wait for the device and returns PSAMD_ERR_STATE under
 * a capture -- and it never grows, its size depends on the container alone; every later call may be captured into a graph.
 * Contexts that never call pay nothing.
 *
 * Bounded loops.  The groups are found by a union-find over the owned slots whose every write is an atomicMin: a word never
 * rises, every step of a find or a union moves to a strictly smaller slot, and a loop therefore ends by itself whatever the
 * other waves do -- there is no lock, no wait on another thread's word and no grid barrier (groups.hip states the argument).
 * On top of that a union stops after slots_total steps and counts itself in `unfinished`.  Correct code cannot get there:
 * unfinished != 0 says the library is broken, and then the groups are not to be trusted.
 *
 * Determinism.  Every output word is an integer that depends on the frame and the radius alone; the order in which the waves
 * hook the pairs does not enter.  The same bytes from run to run, with graphs or without.
 *
 * Cost on an MI355X at N = 2^20 on 16^3 cells, 321 502 live in 2 997 648 owned slots, 23 632 of them members -- the others
 * are kids on that frame (scripts/groups_cost.py; profiles/groups_cost.txt), measured: 0.66 ms at radius 0.4 (22 981 groups,
 * 673 links), 0.66 ms at 1.0 (17 072 groups, 8 259 links) and 0.88 ms at cell_size (one group, 405 285 links) for the record
 * alone, 0.01 ms more with group[] and both tables; psamd_neighbours' count-and-offsets call beside it 0.81, 0.82 and 0.83 ms
 * (a host clock around the call plus psamd_synchronize, the stream idle before it).  The walk costs the same at every radius;
 * what grows with the radius is the hooking of many links into few roots.
 *
 * PSAMD_ERR_INVALID_ARG: a NULL context or spec, unknown flag bits, a bad radius, capacity < 0 or group_capacity < 0, group,
 * group_first or group_size not 4-byte aligned, result_dev not 8-byte aligned.
 *
 * psamd_groups_result_get: the last call's record, into host memory; waits for the context's stream.
 * psamd_download_groups: the host form -- the same passes staged on the device, then what was asked for copied into host
 * arrays (any may be NULL) of capacity and group_capacity entries: the first min(live, capacity) entries of group, the first
 * min(groups, group_capacity) of the tables; waits for the stream. */
int psamd_groups(psamd_ctx *ctx, const psamd_groups_spec *spec);
int psamd_groups_result_get(psamd_ctx *ctx, psamd_groups_result *out);
int psamd_download_groups(psamd_ctx *ctx, uint32_t flags, float radius, int32_t *group, int64_t capacity,
                          int32_t *group_first, int32_t *group_size, int64_t group_capacity, psamd_groups_result *result);

/* ---- the k nearest within a radius -------------------------------------------------- */
/* psamd_knn: every listed particle's k nearest neighbours within a radius, ordered by distance, on the device, lined up with
 * psamd_export_live: an adaptive SPH smoothing length (the distance to the 32nd neighbour), a k-th-neighbour density estimate
 * k / (4/3 pi r_k^3), topological flocking (the seven nearest whatever their distance), nearest-neighbour statistics --
 * without the lists of psamd_neighbours and a ragged sort behind them.  Not in the reference; the step's arithmetic is untouched
 * and PSAMD_ABI_VERSION stays 8.
 *
 * Queries, candidates and d2.  psamd_neighbours' rules, word for word: the queries are the listed particles of the context's
 * own cells, a kid queried from its slot's position; the candidates are the 27-cell non-periodic stencil in the reference's
 * order with the list capacities honoured; kids are nobody's neighbour; the own entry is left out by sorted index, so two
 * particles at one point are each other's nearest, at d2 == 0; a hit is d2 <= r2 = RN(radius radius), with the same fp32 d2,
 * never fused.  count below is psamd_neighbours' count: the number of hits.
 *
 * Order.  A row holds the min(count, k) hits that are smallest under the key (d2 as an fp32 value, global slot id), in
 * ascending order of that key: nearest's rule -- "ties to the lower global slot id" -- extended.  An id stands once in the
 * stencil, so the key is a total order on a query's hits: the row does not depend on the walk order, on the launch shape or on
 * k, and row(k) is the first k words of row(k').  With k = 1, who and d2 are psamd_neighbours' nearest and nearest_d2, byte
 * for byte.
 *
 * Outputs.  All optional, in export order: entry o is the o-th live owned particle in ascending global slot id, for the first
 * m = min(live, capacity) of them.
 *     found[o]          min(count, k); -1: a live particle that is in no list of the frame
 *     who[o * k + j]    the j-th nearest neighbour, j < found; the words j >= found of a row are -1
 *     d2[o * k + j]     that pair's d2; the words j >= found are +inf
 * A live particle in no list has found = -1 and a row of -1 / +inf.  A neighbour is named by its global slot id (a halo's
 * particle by the id the halo carried).  With PSAMD_KNN_INDEX it is named by its export index, so that pos[who] is a plain
 * gather once the -1 are masked; an index at or past capacity is kept true.  The order is still by global slot id -- the
 * export order is ascending slot id, so this is the same order.  The index form is served for world == 1 only
 * (PSAMD_ERR_UNSUPPORTED otherwise).
 *
 * What `full` means.  Every particle outside a query's stencil is a cell edge or more away from it.  So with radius ==
 * cell_size, the row of a query that counts in `full` holds its k nearest candidates of the whole non-periodic box -- with
 * psamd_neighbours' caveat at exactly cell_size: a pair a rounding inside the radius across two cell walls is not in the
 * stencil.  A query that does not count in `full` says the cap -- the radius -- was hit, not that nobody else is near.
 *
 * Record.  listed: the queries, psamd_neighbours'; found: the sum over the queries of min(count, k), the whole context's
 * whatever the capacity; full: the queries with count >= k; k; dk2_min and dk2_max: the smallest and the largest d2 of a k-th
 * neighbour over the full queries, +inf and -inf if there is none.  found and full are integer sums, dk2_min and dk2_max a
 * minimum and a maximum of fp32 values: any reduction tree gives the same words.  A slab world's records combine: the counts
 * add, dk2_min takes the minimum, dk2_max the maximum.
 *
 * Window, refusals, stream and determinism: psamd_neighbours'.  world == 1: from psamd_build_grid until the frame ends;
 * world > 1: between psamd_slab_pairs and psamd_slab_apply, on a plan that lends nothing; a lending plan and an all-pairs world
 * return PSAMD_ERR_UNSUPPORTED and leave the context usable; elsewhere and on a wedged context PSAMD_ERR_STATE.  The call is
 * served on every force model and writes nothing of the frame, the force records or the step.  Everything is enqueued on the
 * context's stream; nothing waits, nothing is read back.  The scratch (the slot -> export index table and a few words per
 * walk task) is the context's: the first call allocates it -- that call may wait for the device and returns PSAMD_ERR_STATE
 * under a capture -- and it never grows: its size depends on the container alone and never on k, the rows go straight to the
 * caller's arrays; every later call may be captured into a graph.  Contexts that never call pay nothing.  Every output word
 * is an integer or one fp32 value with a fixed operand order: the same bytes from run to run, with graphs or without; by id,
 * the union of a slab world's rows is the single context's byte for byte.
 *
 * Cost on an MI355X at N = 2^20 on 16^3 cells, 321 502 live in 2 997 648 owned slots (scripts/knn_cost.py;
 * profiles/knn_cost.txt), measured: psamd_knn with found and the rows 0.86 ms at k = 1, 0.91 ms at k = 8 and
 * 1.60 ms at k = 32 at radius 1.0 (found 55 915, 78 242 and 78 260), 0.88, 1.00 and 2.26 ms at cell_size (found 316 611, 2 413 297
 * and 7 684 457; 109 241 of the 321 502 queries full at k = 32); the record alone 0.12 ms less at k = 32 and within 0.03 ms at
 * k <= 8.  Beside them in the same run psamd_neighbours' count-and-offsets call 0.81 and 0.84 ms -- the same walk, which k = 1
 * stays within 0.05 ms of -- and its with-lists call 1.37 and 1.39 ms, today's route before its ragged sort and the figure to
 * beat: k = 1 and k = 8 beat it, k = 32 does not.  On this frame a row of 32 almost never fills, so the reject in front of
 * the insertion never closes and every hit of any lane sends its whole wave through the 32-position sweep; that kernel also
 * runs at 5 waves per SIMD instead of 8 (a host clock around the call plus psamd_synchronize, the stream idle before it).
 *
 * PSAMD_ERR_INVALID_ARG: a NULL context or spec, unknown flag bits, reserved != 0, a bad radius, k outside 1 ..
 * PSAMD_KNN_MAX_K, capacity < 0 or capacity * k not below 2^62, found, who or d2 not 4-byte aligned, result_dev not 8-byte
 * aligned.
 *
 * psamd_knn_result_get: the last call's record, into host memory; waits for the context's stream.
 * psamd_download_knn: the host form -- the same passes staged on the device (the staging holds min(capacity, owned slots)
 * rows: give a capacity near the live count), then what was asked for copied into host arrays (any may be NULL) of capacity
 * and capacity * k entries; waits for the stream. */
int psamd_knn(psamd_ctx *ctx, const psamd_knn_spec *spec);
int psamd_knn_result_get(psamd_ctx *ctx, psamd_knn_result *out);
int psamd_download_knn(psamd_ctx *ctx, uint32_t flags, float radius, int32_t k, int32_t *found, int32_t *who, float *d2,
                       int64_t capacity, psamd_knn_result *result);

/* ---- long-range gravity (PSAMD_FLAG_FAR_MONOPOLE) ------------------------------ */
/* The cutoff pass leaves most of a long-range force out; PSAMD_FLAG_ALL_PAIRS has all of it at O(N^2).  With this flag a
 * particle's acceleration is the stencil's chain, exactly the cutoff pass's, plus ONE body per cell beyond its stencil.  Not
 * in the reference; everything after the pair stage is untouched.
 *
 * Moments.  In the pair stage, from the snapshot psamd_build_grid left: cell c's moments come from the first
 * min(count, MAX_PARTICLES_PER_CELL) entries of c in the sorted snapshot with the w_eff the force pass uses (0 for a kid,
 * force_sign folded in).  In fp64, S = sum w_eff and Sx = sum w_eff*x, Sy, Sz likewise: the additions run in LIST ORDER,
 * entry 0 first, one addition per entry, every sum started at +0; each product of two fp32 values is exact in fp64, so a
 * fused multiply-add changes nothing.  M_c = (float)S, X_c = (float)(Sx / S), Y_c and Z_c likewise (fp64 division, one
 * rounding to fp32).  If S == 0 -- an empty cell, or kids only -- M_c = X_c = Y_c = Z_c = 0.  A host that repeats these
 * operations gets the same bits (tests/far_model.py does).
 *
 * Far acceleration.  For every particle the force pass serves (no kid, no collision this step), in cell c_i: the cells of
 * the box are walked in global index order; a cell contributes the one body (X_c, Y_c, Z_c, M_c) through the context's own
 * pair form -- the exact lean forms of the force pass, or the fast ones on a PSAMD_FLAG_FAST_MATH context.  A cell of c_i's own
 * non-periodic 27-cell stencil contributes nothing (the cutoff pass has its bodies one by one), and neither does a cell with
 * M_c == 0: they are left out or entered with mass 0, which gives the same bits -- a chain that starts at +0 never becomes -0.
 *
 * Association.  The cells go by blocks of 64 consecutive global indices (block b: cells 64 b .. 64 b + 63, the last one
 * ragged).  A block's terms are ONE fp32 chain per component that starts at +0, in index order.  The blocks are dealt to 16
 * parts -- part p holds the blocks [floor(nblk * p / 16), floor(nblk * (p + 1) / 16)) of nblk -- and a part's sum is the
 * chain sums added in block order to +0.  The particle's record is (((stencil chain + part 0) + part 1) + ...) + part 15: the
 * all-pairs far pass's scheme.  It depends on G and the global cell order alone -- not on the launch shape, the other
 * particles, graphs on or off, run-ahead, or any max_count-like size: the same bytes from run to run.
 *
 * Consequences.  A cloud inside a 2x2x2 block of cells has no far cell: the force records and the whole step are the cutoff
 * context's, byte for byte.  A frame with at most one adult per cell has X_c equal to that adult's position and M_c equal to
 * its w_eff exactly, and the result is the all-pairs force up to association.
 *
 * Accuracy (an fp64 model of the method against an fp64 direct sum, 8192 bodies on 8^3 cells, uniform and clustered): the
 * median particle's |a| is off by 0.2 %, the worst by 1-2 %; the cutoff alone leaves out 77-89 % for the median particle
 * (tests/test_far_monopole_cpu.py).  The device follows the model to 1e-5 relative (tests/test_gpu_far_monopole.py).
 *
 * Refusals.  psamd_create: with PSAMD_FLAG_ALL_PAIRS PSAMD_ERR_INVALID_ARG; with world > 1 and without PSAMD_FLAG_FAR_SLAB, with a softening length outside
 * the lean range, or without the two-pass pair stage (collision radius not small against the cell) PSAMD_ERR_UNSUPPORTED.
 * psamd_potential, psamd_download_potential and psamd_probe without PSAMD_POTENTIAL_FAR / PSAMD_PROBE_FAR return
 * PSAMD_ERR_UNSUPPORTED on such a context, which stays usable: they promise exactly the stencil's bodies, and that is not this
 * context's field.  With the bit (psamd_download_potential_far for the host form) they serve the stencil and then every cell
 * beyond it as one body, formed from the frame's snapshot by the call itself ("energy", "the field at chosen points").  The flag combines
 * freely with FAST_MATH, EULER, EXPLOSIONS, drag, force_sign, graphs, run-ahead and snapshot save / restore.
 *
 * Cost on an MI355X at N = 2^20, default constants (profiles/far_monopole_cost.txt): a step takes 6.43 ms with the flag, 2.17 ms without it (the cutoff step) and 285.9 ms with PSAMD_FLAG_ALL_PAIRS: 2.96 times the cutoff step, 44 times faster than all-pairs;
 * 200 served particles against an fp64 direct sum over all 2^20 bodies: |a| off by 0.034 % for the median particle and 0.21 % for the worst, where the cutoff's records are off by 97.5 % (median).  The pair stage's own timer: 3.68 ms against 1.85 ms.
 *
 * psamd_download_cell_moments: float4[num_cells] = (X_c, Y_c, Z_c, M_c) of the frame, by global cell.  Valid from
 * psamd_calc_forces_pairs until the frame ends (psamd_step cannot be interposed: use the stage calls); elsewhere
 * PSAMD_ERR_STATE.  On a context without the flag PSAMD_ERR_UNSUPPORTED.  Waits for the context's stream. */
int psamd_download_cell_moments(psamd_ctx *ctx, void *out_float4);

/* ---- a pyramid of monopoles (PSAMD_FLAG_FAR_PYRAMID) ---------------------------- */
/* PSAMD_FLAG_FAR_MONOPOLE enters G^3 - 27 bodies per particle.  Most of them are distant and can be merged: with this flag
 * farther mass comes in coarser cells, and a particle's far bodies grow with log G (about 300 on 16^3 cells, 500 on 40^3).  A force model of its
 * own: contexts without the flag, PSAMD_FLAG_FAR_MONOPOLE contexts included, compute what they did.  Not in the reference.
 *
 * Levels.  Level 0 is the cell grid, G_0 = G.  Level l + 1 has G_{l+1} = ceil(G_l / 2) cells per axis.  The top level L is
 * the first with G_L <= 4 (16 -> 8 -> 4: L = 2; 10 -> 5 -> 3: L = 2; G <= 4: L = 0).  The cell with coordinates (i1, i2, i3)
 * lies in the level-l cell (i1 >> l, i2 >> l, i3 >> l); level-l cells are numbered (k3 * G_l + k1) * G_l + k2, like cells.
 * (The packed cell coordinates are 10 bits each: G <= 1023, at most 9 levels.)
 *
 * Moments.  Level 0 is exactly PSAMD_FLAG_FAR_MONOPOLE's: the fp64 sums S, Sx, Sy, Sz over the first
 * min(count, MAX_PARTICLES_PER_CELL) entries of the cell in list order, with the force pass's w_eff; the fp64 sums are kept.
 * A level-(l+1) cell's four fp64 sums are its existing children's fp64 sums, added one at a time in ascending child index,
 * each sum started at +0 (additions only: contraction cannot matter).  At every level M = (float)S, X = (float)(Sx / S), Y
 * and Z likewise; S == 0 gives four zeros.  A host that repeats this gets the same bits (tests/far_model.py does).
 *
 * Interaction set of a particle in cell i that the force pass serves (no kid, no collision this step):
 *   at the top level, every level-L cell J with max-norm |J - (i >> L)| > 1;
 *   at each level l < L, every level-l cell J whose parent is within 1 of i's parent, |(J >> 1) - (i >> (l + 1))| <= 1, and
 *   which itself is not within 1 of i >> l.
 * At level 0 "not within 1" is "not in the stencil": the cutoff pass has those bodies one by one.  Every cell of the box is
 * thus covered exactly once: by the stencil, or by exactly one ancestor in the set.  A body of mass 0 contributes nothing.
 * Each body goes through the context's own pair form (the exact lean form, or the fast one with PSAMD_FLAG_FAST_MATH).
 *
 * Association, fixed by G and the particle's cell alone.  Within a level the cells go in level index order by blocks of 64
 * consecutive indices; a block is ONE fp32 chain per component started at +0; a level's sum is its block chains added in
 * block order to +0.  The record is ((stencil chain + level L) + level L-1) + ... + level 0.  Cells outside the set are
 * entered with mass 0 or skipped: the same bits, since a chain that starts at +0 never becomes -0.  Nothing depends on the
 * launch shape, other particles, graphs, run-ahead or any bound: the same bytes from run to run.
 *
 * Consequences.  On a grid with G <= 4 the force records and whole steps are those of a PSAMD_FLAG_FAR_MONOPOLE context,
 * byte for byte (one level, one block; the 15 empty parts there add +0).  A cloud inside a 2x2x2 block of cells gives the
 * cutoff context's bytes: no ancestor of a stencil cell is ever in the set.
 *
 * Accuracy (an fp64 model of the method against an fp64 direct sum, 8192 bodies, uniform and clustered, 400 sampled;
 * tests/test_far_pyramid_cpu.py): the median particle's |a| is off by 0.2-0.5 %, the worst
 * by 2-4.4 % on 8^3 and 10^3 cells (the flat method on 8^3: 0.15-0.2 % and 1.6-3.5 %); the cutoff alone leaves out 77-91 % for the
 * median particle.  A particle's far bodies: 153 of 491 on 8^3 cells, 295 of 4072 on 16^3 in the mean.  The device follows the
 * model to 1e-5 relative (tests/test_gpu_far_pyramid.py).
 *
 * Refusals mirror PSAMD_FLAG_FAR_MONOPOLE's.  psamd_create: with PSAMD_FLAG_ALL_PAIRS or PSAMD_FLAG_FAR_MONOPOLE
 * PSAMD_ERR_INVALID_ARG; with world > 1 and without PSAMD_FLAG_FAR_SLAB, a softening length outside the lean range, or without the two-pass pair stage
 * PSAMD_ERR_UNSUPPORTED.  psamd_potential, psamd_download_potential and psamd_probe without PSAMD_POTENTIAL_FAR /
 * PSAMD_PROBE_FAR return PSAMD_ERR_UNSUPPORTED on such a context, which stays usable; with the bit they serve the stencil and
 * then the interaction set above, levels L down to 0, from moments the call forms itself.  The flag combines freely with FAST_MATH, EULER, EXPLOSIONS, drag, force_sign, graphs,
 * run-ahead and snapshot save / restore.
 *
 * Cost on an MI355X, default constants (profiles/far_pyramid_cost.txt): at N = 2^20 (16^3 cells) a step takes 6.19 ms with the flag, 6.43 ms with
 * PSAMD_FLAG_FAR_MONOPOLE and 2.18 ms with neither (the pair stage's own timer: 3.46, 3.67 and 1.86 ms); at N = 2^22 (24^3 cells)
 * 18.6, 27.9 and 9.3 ms (14.8, 24.4 and 8.5 ms).  200 served particles against an fp64 direct sum over all bodies: |a| off by
 * 0.057 % for the median particle and 0.48 % for the worst at 2^20 (the flat method: 0.034 % and 0.21 %), 0.059 % and 0.21 % at 2^22
 * (0.020 % and 0.13 %).  A fourteenth of the far bodies buys 4 % of the step at 16^3 and a third at 24^3: the walk is bound by
 * scanning the blocks of its box, not by its pairs (by its structure; not profiled).
 *
 * psamd_far_levels: host only, no device.  *levels = L + 1, dims[0 .. L] = G_0 .. G_L, the rest of dims 0.
 * psamd_download_level_moments: float4[G_level^3] = (X, Y, Z, M) of one level of the frame, by level cell index.  The validity
 * window and error codes of psamd_download_cell_moments; a level outside [0, L] PSAMD_ERR_INVALID_ARG; on a context without
 * PSAMD_FLAG_FAR_PYRAMID PSAMD_ERR_UNSUPPORTED.  Waits for the context's stream.  psamd_download_cell_moments also works on a
 * pyramid context, where it returns level 0. */
int psamd_far_levels(const psamd_config *cfg, int32_t *levels, int32_t dims[16]);
int psamd_download_level_moments(psamd_ctx *ctx, int32_t level, void *out_float4);

/* ---- quadrupoles on the pyramid (PSAMD_FLAG_FAR_QUADRUPOLE) ---------------------- */
/* The pyramid enters a level-l cell as a point mass at distances of only two of its own edges, and that is what its error
 * is made of.  With this flag, a modifier of PSAMD_FLAG_FAR_PYRAMID, every cell of every level also carries its second moments
 * and every far body adds its quadrupole term.  The interaction set, the members, the blocks, the levels and every monopole
 * term are the pyramid's; contexts without the flag compute what they did, in the same bytes.
 *
 * Moments.  Ten fp64 sums per cell of every level: S, Sx, Sy, Sz as on the pyramid (the same bits) and six raw second
 * moments S_ab in the plane order (a, b) = xx, yy, zz, xy, xz, yz.  Level 0: over the first min(count,
 * MAX_PARTICLES_PER_CELL) entries in list order, every sum started at +0, one addition per entry; the term of entry j is
 * RN(RN(w_eff * x_a) * x_b) -- the inner product is exact in fp64, the outer one is ONE fp64 rounding; no operation is fused.
 * Level l + 1: the children's sums added in ascending child index to +0 (raw moments about the origin need no shift).
 * At every level, in fp64 and unfused, C_ab = (float)(S_ab - RN(RN(S_a / S) * S_b)), a the first index of the plane's name;
 * S == 0 gives six zeros.  A cell with one adult gives six exact zeros (both products round the same real number).  M, X, Y,
 * Z are the pyramid context's bit for bit.  A host that repeats this gets the same bits (tests/far_model.py does).
 *
 * The quadrupole term of a member (X, Y, Z, M != 0, C) on a particle at x: the second-order Taylor term of the softened
 * kernel about the centre of mass (the first-order term vanishes there),
 *     a_q = -3 (C d) u^5 + 7.5 (d.C.d) u^7 d - 1.5 T u^5 d,    d = (X, Y, Z) - x,  u = (d.d + eps2)^(-1/2),  T = Cxx + Cyy + Czz.
 * In fp32, the same operations on exact and PSAMD_FLAG_FAST_MATH contexts, every product and sum rounded once unless it is
 * written fma (one rounding for a * b + c):
 *     dx = X - x,  dy = Y - y,  dz = Z - z
 *     r2 = (dx*dx + dy*dy) + dz*dz                      u  = rsq(r2 + eps2)      (the hardware reciprocal square root, 1 ulp)
 *     u2 = u*u,  u3 = u2*u,  u5 = u3*u2,  u7 = u5*u2
 *     gx = fma(Cxz, dz, fma(Cxy, dy, Cxx*dx))           gy = fma(Cyz, dz, fma(Cyy, dy, Cxy*dx))
 *     gz = fma(Czz, dz, fma(Cyz, dy, Cxz*dx))           q  = fma(gz, dz, fma(gy, dy, gx*dx))
 *     T  = (Cxx + Cyy) + Czz                            s  = fma(7.5*u7, q, (-1.5*T)*u5)       m3 = -3*u5
 *     a_q = (fma(m3, gx, s*dx), fma(m3, gy, s*dy), fma(m3, gz, s*dz))
 * The far potential and the far probes of such a context (PSAMD_POTENTIAL_QUADRUPOLE, PSAMD_PROBE_QUADRUPOLE) repeat this
 * sequence up to q and T -- u7 apart -- and form the potential's term from it, in the convention of the potential's sums (sum of
 * w u, phi = -sum):
 *     t_q = fma(1.5*u5, q, (-0.5*T)*u3)                                    (= 1.5 (d.C.d) u^5 - 0.5 T u^3; its gradient is a_q)
 * A probe's acceleration term is a_q above, operation for operation.
 *
 * Association.  Within a block of 64 level cells the quadrupole terms form their OWN fp32 chain per component: from +0, in
 * index order, over the members of the monopole chain.  A level's quadrupole sum is its blocks' quadrupole chains added in
 * block order to +0; the level's part is RN(monopole sum + quadrupole sum) per component, and the record is
 * ((stencil + part L) + ...) + part 0 as on the pyramid.  A cell outside a particle's set is skipped or adds +0: the same
 * bits.  Nothing depends on the launch shape, other particles, graphs or run-ahead.
 *
 * Consequences.  A cloud inside a 2x2x2 block of cells gives the cutoff context's bytes.  On G <= 4 with at most one adult per
 * cell (kids anywhere) every C is an exact zero and every quadrupole chain is +0: records and whole steps are the
 * PSAMD_FLAG_FAR_PYRAMID context's, byte for byte.
 *
 * Accuracy (an fp64 model of the method against an fp64 direct sum, the clouds of tests/test_far_pyramid_cpu.py;
 * tests/test_far_quadrupole_cpu.py): the median particle's |a| is off by 0.07-0.11 %, the worst by 0.5-1.7 % on 8^3 and
 * 10^3 cells, where the pyramid of monopoles is off by 0.2-0.5 % and 1.9-4.4 %: the median falls to 0.21-0.35 of the pyramid's.
 * The device follows the model to 1e-5 relative (tests/test_gpu_far_quadrupole.py).
 *
 * Refusals.  psamd_create: the flag without PSAMD_FLAG_FAR_PYRAMID PSAMD_ERR_INVALID_ARG; everything else as the pyramid
 * refuses it.  psamd_potential, psamd_download_potential, psamd_download_potential_far and psamd_probe return
 * PSAMD_ERR_UNSUPPORTED on such a context without a modifier and with PSAMD_POTENTIAL_FAR / PSAMD_PROBE_FAR alone, and the
 * context stays usable: those far forms are monopoles only, which is not this context's field.  Its own field is served where
 * it is asked for by name: PSAMD_POTENTIAL_FAR | PSAMD_POTENTIAL_QUADRUPOLE (host form: psamd_download_potential_flags) and
 * PSAMD_PROBE_FAR | PSAMD_PROBE_QUADRUPOLE ("energy", "the field at chosen points"); either quadrupole bit without its FAR bit is
 * PSAMD_ERR_INVALID_ARG, and on a context without the flag both are unknown bits.  The flag combines with FAST_MATH, EULER,
 * EXPLOSIONS, drag, force_sign, graphs, run-ahead and snapshot save / restore as the pyramid does.
 *
 * Cost on an MI355X (profiles/far_quadrupole_cost.txt): at N = 2^20 (16^3 cells) a step takes 7.27 ms with the flag against 6.22 ms
 * for the pyramid of monopoles in the same run and 2.18 ms for the cutoff step (the pair stage's own timer: 4.59, 3.49 and
 * 1.88 ms): 1.17 times the pyramid step.  At N = 2^22 (24^3 cells) 23.6 ms against 18.7 ms and 9.4 ms (19.7, 15.0 and 8.5 ms):
 * 1.26 times.  200 served particles against an fp64 direct sum over all bodies: |a| off by 0.037 % for the median particle and
 * 0.14 % for the worst at 2^20 (the pyramid: 0.057 % and 0.48 %), 0.047 % and 0.11 % at 2^22 (0.059 % and 0.21 %).  The far
 * work grows 1.7 times: with the quadrupole term the pairs weigh as much as the scan of the blocks (not profiled).
 *
 * psamd_download_level_quadrupoles: float[G_level^3][6] = (Cxx, Cyy, Czz, Cxy, Cxz, Cyz) of one level of the frame, by level
 * cell index.  The validity window and error codes of psamd_download_level_moments; NULL arguments or a level outside [0, L]
 * PSAMD_ERR_INVALID_ARG; on a context without the flag PSAMD_ERR_UNSUPPORTED.  Waits for the context's stream. */
int psamd_download_level_quadrupoles(psamd_ctx *ctx, int32_t level, void *out_float6);

/* ---- far field on slabs (PSAMD_FLAG_FAR_SLAB) ----------------------------------- */
/* The far field of PSAMD_FLAG_FAR_MONOPOLE and PSAMD_FLAG_FAR_PYRAMID (with or without PSAMD_FLAG_FAR_QUADRUPOLE) on the slab
 * partition.  A rank needs its neighbours' halos, which it has, and the moments of every cell of the box: 32 or 80 bytes a
 * cell.  The moments of a cell depend on the cell's own list alone, the far set of a particle on G and its cell alone, and the
 * sums are fp64 sums in list order: the union of the ranks is one context's state, byte for byte, every step
 * (tests/test_gpu_far_slab.py).
 *
 * The flag.  A far slab has one more message that must be all-gathered between psamd_slab_build and psamd_slab_pairs; a host
 * written for the cutoff exchange that does not carry it would step with stale moments.  With the bit the host has said that it
 * gathers.  Without it a far flag with world > 1 stays PSAMD_ERR_UNSUPPORTED; with it and world > 1 the context is created (the
 * lean-range, two-pass and all-pairs refusals stay); with it and world == 1 no message exists and every byte is what the context
 * computes without it; the flag with neither far flag is PSAMD_ERR_INVALID_ARG.  PSAMD_ABI_VERSION stays 8: the bit is additive.
 *
 * The message: allg_out / allg_in, the all-pairs slot (a context is never both).  allg_out, written by psamd_slab_build: 16
 * header words -- [0] the rank's own cells (those of its state layers), [1] the planes, 4 or 10, [2] the sender's sticky error
 * bits, [3] its first global cell -- then, 8-byte aligned, planes x allg_cells doubles, plane-major: S, Sx, Sy, Sz and with
 * quadrupoles Sxx, Syy, Szz, Sxy, Sxz, Syz; a cell's index in a plane is its local index.  allg_cells is the largest state-layer
 * cell count over all ranks, so allg_bytes = 64 + planes * allg_cells * 8 is the same on every rank under uneven cuts (the
 * header is 64 bytes: nothing is rounded).  The sums are the one-context sums of "long-range gravity" and "quadrupoles on the
 * pyramid": the first min(count, MAX_PARTICLES_PER_CELL) entries, list order, one addition per entry, unfused.
 *
 * psamd_slab_pairs checks every block's header against the plan of its rank (cells, first cell, planes), adopts the senders'
 * error bits, scatters the sums to level 0 by global cell, forms level 0's X, Y, Z, M (and C) from them by the one-context
 * operations and adds up the levels above: every rank builds the upper levels redundantly, O(cells).  A block that did not
 * arrive or is another context's fails the step collectively ("a slab message does not match"), and is never followed: the
 * plan's numbers bound every index.  A stale but well-formed block of the step before is NOT detected, as for all-pairs.
 * There is no interior pass: psamd_slab_pairs_interior returns PSAMD_OK and does nothing (the far pass needs the gather).
 * The records of lent layers travel home in force_out as they do on every slab.
 *
 * Downloads.  psamd_download_cell_moments, psamd_download_level_moments and psamd_download_level_quadrupoles are valid from
 * psamd_slab_pairs until the frame ends; every rank returns the arrays of the whole box.
 *
 * Not served with world > 1, whatever bits are set: psamd_potential, psamd_download_potential and its _far and _flags forms,
 * psamd_probe return PSAMD_ERR_UNSUPPORTED and the context stays usable.  Far slabs combine with FAST_MATH, EULER, EXPLOSIONS,
 * drag, force_sign, graphs and run-ahead as slabs and far contexts do.
 *
 * Cost (scripts/far_slab_cost.py; profiles/far_slab_cost.txt): no machine with several GPUs was at hand, so the eight-rank
 * figures there are projections from eight slabs stepped on ONE MI355X, as in DESIGN.md section 6. */

/* ---- introspection -------------------------------------------------------- */
int psamd_get_counters(psamd_ctx *ctx, psamd_counters *out);
int psamd_live_count(psamd_ctx *ctx, int64_t *out);
int psamd_device_view_get(psamd_ctx *ctx, psamd_device_view *out);
/* Diagnostic builds (-DPSAMD_WAVE_TRACE) record per pair-kernel wave: start, end
 * (100 MHz real-time counter) and hardware id; 3 words per wave slot.  Zeros otherwise. */
int psamd_debug_wave_trace(psamd_ctx *ctx, uint64_t *out, int64_t n_words);
/* The packs of partly filled last slices of the frame's last pair stage (between psamd_calc_forces_pairs and the frame's
 * end; the scalar walk of the two-pass stage has them, every other launch shape has none): *count packs, the first
 * min(*count, capacity) of them as four cell numbers each in `cells` (-1: unused place), in pack order.  *shape (may be
 * NULL): how that pair stage was launched -- wave slots / 32 in bits 0-9, bit 10 the tile walk (no packs), bit 11 the
 * two-pass stage, from bit 12 the pack workgroups / 8.  Waits for the context's stream. */
int psamd_debug_packs(psamd_ctx *ctx, int32_t *cells, int64_t capacity, int64_t *count, uint64_t *shape);

/* Exhaustive check of the hand-written correctly rounded fp32 sqrt / reciprocal used by
 * the pair kernel against the compiler's forms, over every float with bit pattern in
 * [lo_bits, hi_bits].  out24[0..2] = mismatches of the sqrt, the reciprocal and their
 * composition RN(1/RN(sqrt x)) as used; [3] = mismatches of a rejected shortcut (for the
 * record); [8..15], [16..23] = first offending inputs of the sqrt and the composition. */
int psamd_selftest_math(psamd_ctx *ctx, uint32_t lo_bits, uint32_t hi_bits, uint64_t out24[24]);
/* Device time per kernel group, accumulated over the steps since psamd_set_timing, in
 * microseconds, measured with HIP events on the context's stream: hist, scan, scatter,
 * sort, pairs (the force pass), apply, lifecycle, frame reset, collide (collision flags and the
 * lists of the particles that need a force: the two-pass prologue of the pair stage).  level 0: off; 1: collide, pairs, apply and lifecycle
 * only (four events per step); 2: every stage (an event between two kernels costs a few
 * microseconds of idle GPU, so this is for diagnosis).  Never makes a step wait: a step's events are read two timed
 * steps later, or by psamd_get_timing.
 * psamd_set_timing_period(ctx, n): record the events on every n-th step only (n >= 1; default 1) --
 * the accumulated times and `launches` then count those steps; what a long timed run uses so that
 * the events' idle gaps (four to six per step at level 1) do not weigh on the steps in between. */
#define PSAMD_NUM_TIMERS 9
int psamd_set_timing(psamd_ctx *ctx, int level);
int psamd_set_timing_period(psamd_ctx *ctx, int every);
int psamd_get_timing(psamd_ctx *ctx, double us_out[PSAMD_NUM_TIMERS], int64_t *launches);
/* the same intervals as a distribution over the timed steps: median and maximum per timer (a mean hides a stall) */
int psamd_get_timing_stats(psamd_ctx *ctx, double median_us[PSAMD_NUM_TIMERS], double max_us[PSAMD_NUM_TIMERS], int64_t *samples);

#ifdef __cplusplus
}
#endif
#endif /* PSAMD_H */
