/*
 * include/hdd.h -- C ABI of the MI355X SWIPDG assembly engine (libhdd_amd.so).
 *
 * Drop-in boundary for dune-hdd's linearelliptic SWIPDG / BlockSWIPDG hot path.  The reference has no
 * C ABI (its boundary is C++ templates over dune-gdt's SystemAssembler); every entry point below names
 * the reference interface it replaces.  Conventions:
 *   - plain C types and pointers only; "device" pointers are HIP device memory owned by the caller;
 *   - every function returns HDD_OK (0) or an HDD_ERR_* code, never throws; hdd_last_error(ctx) (or
 *     hdd_last_error(NULL) for functions without a context) returns the message of the last failure
 *     of the calling thread;
 *   - device work is enqueued on the hipStream_t passed as `stream` (NULL = legacy default stream) and
 *     is NOT synchronised; no synchronisation happens inside hdd_swipdg_assemble / hdd_affine_lincomb /
 *     hdd_soa_gather / hdd_soa_scatter, and no allocation either except that hdd_swipdg_assemble on
 *     HDD_HEX p=3 meshes grows a context-owned workspace the first time a context sees a larger mesh --
 *     8 * (72 n + 1280 ceil(n / 16) + 2 n) bytes for n owned elements (the 576-byte element records, the
 *     GEMM coefficient fragments of 80 doubles per element padded to groups of 16, 16 bytes of layout per
 *     element; ~1.23 KB per element) -- and allocates, on its first p=3 call, the context's 80 x 4096 table
 *     of reference matrices (2.6 MB): warm a context up once, then the calls are hipGraph-capturable;
 *   - one context per thread at a time (thread-compatible, like the reference's single-threaded init()),
 *     and one stream at a time per context: the HDD_HEX p=3 coefficient records live in a per-context
 *     workspace, so concurrent assemblies on different streams need different contexts.
 *
 * Numbering: DoF (row / column) of local basis function i of element g is g*nb + i (element-blocked,
 * as dune-fem's DG mapper); a CSR row holds the DoFs of its element and of every face neighbour, sorted
 * ascending (the EllipticSWIPDG pattern, swipdg.hh:169).  Block-SWIPDG numbering is the same rule applied
 * to a subdomain-major element order (Spaces::Block::mapToGlobal(ss, ii) = offset(ss) + ii,
 * block-swipdg.hh:1042, 1093), which all hdd_grid_* builders produce.
 */
#ifndef HDD_H
#define HDD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HDD_ABI_VERSION 8   /* 3: hdd_mesh vertex-indexed geometry, hdd_local_vertices;
                               4: HDD_FN_FLATTOP (hdd_scalar_fn.table / n_table), hdd_indicator_sum;
                               5: hdd_shard_info.halo_elements, hdd_swipdg_assemble_elements;
                               6: hdd_grid_create_hex_from_connectivity;
                               7: in-process device transport (hdd_device_hub, hdd_comm_create_device);
                               8: sharded-step watchdog (hdd_block_step_mark / _query / _sync, HDD_ERR_TIMEOUT), the
                                  device transport's stall injection, verification variants (hdd_ctx_set_variant) */
#define HDD_MAX_COMP 8

typedef enum {
  HDD_OK = 0,
  HDD_ERR_INVALID = 1,      /* wrong input given (Stuff::Exceptions::wrong_input_given) */
  HDD_ERR_HIP = 2,          /* HIP runtime failure */
  HDD_ERR_UNSUPPORTED = 3,  /* NotImplemented in the reference's sense */
  HDD_ERR_NOMEM = 4,
  HDD_ERR_RANGE = 5,        /* index_out_of_range */
  HDD_ERR_TIMEOUT = 6       /* a deadline passed (hdd_block_step_sync: a sharded step that did not complete) */
} hdd_status;

enum { HDD_SIMPLEX = 0, HDD_CUBE = 1,                       /* P1 triangles / Q1 parallelograms (2d) */
       HDD_HEX = 2 };                                        /* Q_p (p = 1..3) on affine hexahedra (3d) */
enum { HDD_NBR_DIRICHLET = -1, HDD_NBR_NEUMANN = -2 };       /* neighbour codes of domain-boundary faces */
enum { HDD_FN_CONST = 0, HDD_FN_PER_ELEM = 1, HDD_FN_SINUSOID = 2, HDD_FN_COS_PRODUCT = 3, HDD_FN_FLATTOP = 4 };
#define HDD_FLATTOP_REC 7      /* doubles per HDD_FN_FLATTOP box: lx, ly, ux, uy, layer_x, layer_y, value */
enum { HDD_TENSOR_CONST = 0, HDD_TENSOR_ISO_PER_ELEM = 1, HDD_TENSOR_SYM_PER_ELEM = 2 };
enum { HDD_BOUNDARY_ALL_DIRICHLET = 0, HDD_BOUNDARY_ALL_NEUMANN = 1 };

typedef struct hdd_ctx hdd_ctx;
typedef struct hdd_grid hdd_grid;
typedef struct hdd_local hdd_local;

/* ---------------------------------------------------------------------------------------------- */
/* context                                                                                         */
/* ---------------------------------------------------------------------------------------------- */
int hdd_abi_version(void);
/* binds `hip_device`; replaces nothing in the reference (DUNE is host-only) */
int hdd_ctx_create(int hip_device, hdd_ctx** out);
void hdd_ctx_destroy(hdd_ctx* ctx);
/* error injection of the tests (the HDD_DEBUG_FLAGS value a context reads at creation; 0 in production).
 * Bit 524288: hdd_swipdg_rhs's face launch is treated as failed (the call returns HDD_ERR_HIP after its volume
 * kernel; the next call must still be correct).  Profiling ablations exist only in the separate -DHDD_ABLATION
 * build (make ablation: lib_ab/libhdd_abl.so); the product library ignores every other bit. */
int hdd_ctx_set_debug_flags(hdd_ctx* ctx, int32_t flags);
/* Verification variants (ABI 8): alternative implementations of the same values, selected per context (or by the
 * HDD_VARIANT value a context of the -DHDD_ABLATION build reads at creation; the product library takes no kernel
 * choice from the environment) so that the tests can compare them bit for bit / to rounding with the default kernels.  Default 0: the kernels the dispatch picks for performance. */
enum {
  HDD_VARIANT_Q1_WHOLE_TILE = 1,      /* Q1: the whole-tile image kernel on every mesh (the default on element-major
                                         meshes and on the sharded step's SKIP launches) instead of the half-image one */
  HDD_VARIANT_ELEMENT_MAJOR = 2,      /* ignore the mesh's vertex-indexed geometry (element-major coordinates) */
  HDD_VARIANT_C3_PER_COMPONENT = 4,   /* OS2014 sinusoid components: one launch per component, not the fused one */
  HDD_VARIANT_WAVE_PER_ROW = 8,       /* the generic wave-per-row kernels instead of the persistent tile policies */
  HDD_VARIANT_P1_SMOOTH_QUADRATURE = 16,   /* P1 smooth kappa: the quadrature policy instead of the moments */
  HDD_VARIANT_HEX_Q3_REGISTER = 32,   /* hexahedra p = 3: the register-fragment MFMA kernel, not the GEMM one */
  HDD_VARIANT_PATTERN_SCAN_COPY = 64, /* device pattern nnz by a scan launch + device-to-host copy */
  HDD_VARIANT_RHS_FUSED = 128,        /* 2d RHS: one fused kernel instead of volume kernel + boundary-element list */
  HDD_VARIANT_RHS_GENERIC = 256,      /* RHS: the run-time-rule kernel only */
  HDD_VARIANT_RHS_NO_TINY = 512       /* RHS: no small-phase polynomial tier for the force's cos products */
};
int hdd_ctx_set_variant(hdd_ctx* ctx, uint32_t variant);
/* message of the last failure on this thread (ctx may be NULL); never NULL */
const char* hdd_last_error(const hdd_ctx* ctx);
/* the instantiation name of the last persistent tile kernel this thread launched ("" if none; ABI 8): what the
 * dispatch actually picked, e.g. for a benchmark's kernel label.  Element-list passes are not recorded. */
const char* hdd_last_tile_kernel(void);

/* ---------------------------------------------------------------------------------------------- */
/* grids (host) -- replace the grid providers the reference builds its spaces on:                  */
/*   Stuff::Grid::Providers::Cube (testcases/ESV2007.hh:123-129, testcases/spe10.hh:301-307) and     */
/*   grid::Multiscale::Providers::Cube with num_partitions (testcases/base.hh:150-191)             */
/* ---------------------------------------------------------------------------------------------- */
typedef struct {
  int32_t elem_type;          /* HDD_SIMPLEX: Kuhn split of every square (createSimplexGrid); HDD_CUBE */
  int32_t nx, ny;             /* squares per direction */
  int32_t px, py;             /* subdomain partition ("num_partitions" [px py 1]); 1,1 = monolithic */
  int32_t boundary;           /* HDD_BOUNDARY_* applied to every domain-boundary face */
  int32_t pad;
  double lower[2], upper[2];
} hdd_structured_desc;

/* 3d structured grid of nx x ny x nz axis-aligned hexahedra (SGrid / YaspGrid cube provider in 3d),
 * px x py x pz subdomains (subdomain id (sx*py + sy)*pz + sz: x-slabs are contiguous element ranges);
 * inside a subdomain elements are lexicographic (x fastest).  Faces: 2a (x_a = 0 side), 2a+1. */
typedef struct {
  int32_t nx, ny, nz;
  int32_t px, py, pz;
  int32_t boundary;           /* HDD_BOUNDARY_* */
  int32_t degree;             /* polynomial degree p of the DG Q_p space carried by the grid (1..3) */
  double lower[3], upper[3];
} hdd_structured3_desc;

typedef struct {
  int32_t elem_type, nb, nfaces, nvpe;   /* nb = basis functions per element of the carried DG space */
  int64_t n_elements, n_vertices;
  int32_t n_subdomains, dim;
} hdd_grid_info;

int hdd_grid_create_structured(const hdd_structured_desc* desc, hdd_grid** out);
/* 3d (C5: ESV2007 3d structured, SWIPDG p=3) */
int hdd_grid_create_structured_3d(const hdd_structured3_desc* desc, hdd_grid** out);
/* general conforming 2d mesh from connectivity (vertex order = Dune reference element order);
 * `subdomain` (nullable) assigns elements to subdomains, elements are then renumbered subdomain-major */
int hdd_grid_create_from_connectivity(int32_t elem_type, int64_t n_vertices, const double* vertex_coords,
                                      int64_t n_elements, const int32_t* elem_vert, const int32_t* subdomain,
                                      int32_t n_subdomains, int32_t boundary, hdd_grid** out);
/* general conforming 3d mesh of axis-aligned hexahedra from connectivity (vertex_coords [n_vertices][3],
 * elem_vert [n_elements][8] in Dune cube vertex order: vertex k at lower + ((k&1), (k>>1)&1, k>>2) * h),
 * carrying the DG Q_`degree` space (1..3); shared faces must be aligned (twin face f^1, the layout every
 * subset of a structured hex grid has).  Replaces the grid part the reference hands to an oversampled local
 * discretization in 3d (MsGrid::local_oversampled grid part, block-swipdg.hh:783-817); HDD_ERR_UNSUPPORTED
 * for a non-box element or a misaligned shared face. */
int hdd_grid_create_hex_from_connectivity(int32_t degree, int64_t n_vertices, const double* vertex_coords,
                                          int64_t n_elements, const int32_t* elem_vert, const int32_t* subdomain,
                                          int32_t n_subdomains, int32_t boundary, hdd_grid** out);
void hdd_grid_destroy(hdd_grid* g);
int hdd_grid_get_info(const hdd_grid* g, hdd_grid_info* out);
/* element range [first, last) of the subdomains [s_begin, s_end) in the (subdomain-major) numbering */
int hdd_grid_subdomain_range(const hdd_grid* g, int32_t s_begin, int32_t s_end, int64_t* first, int64_t* last);
/* global element -> (vertex ids [nvpe]) and subdomain ids, for tests / visualisation (host arrays) */
int hdd_grid_connectivity(const hdd_grid* g, double* vertex_coords, int32_t* elem_vert, int32_t* subdomain);

/* Rank-local view: the elements of subdomains [s_begin, s_end) ("owned") plus the ghost elements that
 * share a face with them, laid out [ghosts with smaller global id][owned][ghosts with larger global id]
 * so that local order == global order (owner-computes rows, block-swipdg.hh:355-382). */
typedef struct {
  int64_t n_local, own_begin, own_end, n_ghost;
  int64_t global_first;       /* global id of the first owned element */
} hdd_local_info;

int hdd_local_create(const hdd_grid* g, int32_t s_begin, int32_t s_end, hdd_local** out);
void hdd_local_destroy(hdd_local* l);
int hdd_local_get_info(const hdd_local* l, hdd_local_info* out);
/* host SoA arrays, n_local columns each:
 *   coords    [dim*nvpe][n_local]: coordinate c of vertex k at (dim*k + c)*n_local + e (ghosts too)
 *   neighbors [nfaces][n_local] : local neighbour id or HDD_NBR_* (ghost columns: -3)
 *   face_info [n_local]         : 4 bits per face: twin local face (bits 0-2), reversed (bit 3)
 *   global_id [n_local]         : global element id
 *   subdomain [n_local]         : subdomain of the element
 * any pointer may be NULL */
int hdd_local_fill(const hdd_local* l, double* coords, int32_t* neighbors, uint32_t* face_info,
                   int64_t* global_id, int32_t* subdomain);
/* element barycentres [dim][n_local] (coefficient lookup, e.g. the Spe10 checkerboard) */
int hdd_local_centers(const hdd_local* l, double* centers);
/* vertex-indexed geometry of the local elements (owned + ghosts), the grid's own representation (a Dune
 * grid's vertex set + element -> vertex map): the distinct vertices of the local elements, numbered in
 * ascending global vertex id, *n_vertices of them;
 *   elem_vertices [nvpe][n_local]   : local vertex id of vertex k of element e at k*n_local + e
 *   vertex_coords [n_vertices][dim] : coordinates, interleaved
 * Call with elem_vertices == vertex_coords == NULL to query *n_vertices. */
int hdd_local_vertices(const hdd_local* l, int64_t* n_vertices, int32_t* elem_vertices, double* vertex_coords);
/* halo plan with the subdomain -> rank map `owner` [n_subdomains]:
 *   peers[n_peers] ranks this rank exchanges with (ascending); for peer p: send_count[p] owned elements
 *   whose local ids are listed by hdd_local_send_list(l, p, ...), and recv_count[p] ghost slots starting
 *   at local id recv_offset[p] (ghosts of one owner are contiguous).  Call with peers == NULL to query
 *   n_peers. */
int hdd_local_halo_plan(const hdd_local* l, const int32_t* owner, int32_t my_rank, int32_t* n_peers,
                        int32_t* peers, int64_t* send_count, int64_t* recv_offset, int64_t* recv_count);
int hdd_local_send_list(const hdd_local* l, const int32_t* owner, int32_t my_rank, int32_t peer_index,
                        int32_t* local_ids);

/* dune-stuff Checkerboard evaluated at element barycentres: value of cell (cx, cy), x fastest */
int hdd_checkerboard(int64_t n, const double* centers /*[2][n]*/, const double lower[2], const double upper[2],
                     int32_t ncx, int32_t ncy, const double* cell_values, double* out);
/* dune-stuff Indicator evaluated at element barycentres (problems/spe10.hh:144, 157: the SPE10 channel and
 * force): value of the first closed box [lx, ux] x [ly, uy] containing the barycentre, 0 if none;
 * boxes[5k .. 5k+4] = lx, ly, ux, uy, value */
int hdd_indicator(int64_t n, const double* centers /*[2][n]*/, int32_t n_boxes, const double* boxes, double* out);
/* the sum of one-box Indicators (make_sum of the channel's per-box functions, problems/spe10.hh:139-148 with
 * channel_boundary_layer == 0): sum of the values of every closed box containing the barycentre */
int hdd_indicator_sum(int64_t n, const double* centers /*[2][n]*/, int32_t n_boxes, const double* boxes, double* out);
/* The SPE10 Model1 permeability data file (problems/spe10.hh:151-156: Spe10FunctionType(filename, lower_left,
 * upper_right, model1_min_value, model1_max_value)).  dune-stuff's reader is not in the reference tree; restated
 * (parity unpinned): whitespace-separated numbers, of which the first HDD_SPE10_MODEL1_CELLS (100 x 20, x
 * fastest -- the file holds 6000) are the cells of the 100 x 20 checkerboard, mapped affinely so that
 * [HDD_SPE10_MODEL1_MIN, HDD_SPE10_MODEL1_MAX] goes onto [min_value, max_value] (the identity for the values the
 * reference passes).  cells: [HDD_SPE10_MODEL1_CELLS].  Missing / short file or max_value <= min_value:
 * HDD_ERR_INVALID. */
#define HDD_SPE10_MODEL1_NX 100
#define HDD_SPE10_MODEL1_NZ 20
#define HDD_SPE10_MODEL1_CELLS 2000
#define HDD_SPE10_MODEL1_MIN 0.001
#define HDD_SPE10_MODEL1_MAX 998.915
int hdd_spe10_model1_read(const char* filename, double min_value, double max_value, double* cells);

/* ---------------------------------------------------------------------------------------------- */
/* sparsity pattern (host) -- replaces EllipticSWIPDG::pattern(test, ansatz) (swipdg.hh:169) and the */
/* block pattern of add_local_to_global_pattern / compute_face_pattern (block-swipdg.hh:304-325,     */
/* 1036-1049).  Rows of the owned elements, global columns.                                          */
/* ---------------------------------------------------------------------------------------------- */
int hdd_pattern_count(int32_t elem_type, int64_t n_local, int64_t own_begin, int64_t own_end,
                      const int32_t* neighbors, int64_t* nnz);
/* row_ptr [nb*(own_end-own_begin)+1], col [nnz], elem_ptr [own_end-own_begin+1] (= row_ptr[k*nb]);
 * global_id may be NULL (local == global) */
int hdd_pattern_fill(int32_t elem_type, int64_t n_local, int64_t own_begin, int64_t own_end,
                     const int32_t* neighbors, const int64_t* global_id, int64_t* row_ptr, int32_t* col,
                     int64_t* elem_ptr);
/* the same for any DG space: n_faces faces and nb basis functions per element (Q_p: nb = (p+1)^dim);
 * n_faces = 0 gives the element-local (volume) pattern of the l2 / h1_semi / elliptic / boundary_l2 products */
int hdd_dg_pattern_count(int32_t n_faces, int32_t nb, int64_t n_local, int64_t own_begin, int64_t own_end,
                         const int32_t* neighbors, int64_t* nnz);
int hdd_dg_pattern_fill(int32_t n_faces, int32_t nb, int64_t n_local, int64_t own_begin, int64_t own_end,
                        const int32_t* neighbors, const int64_t* global_id, int64_t* row_ptr, int32_t* col,
                        int64_t* elem_ptr);


/* ---------------------------------------------------------------------------------------------- */
/* device assembly -- replaces the LHS part of SWIPDG::init() (swipdg.hh:222-249 + walk() at 485):   */
/* one GDT::Operators::EllipticSWIPDG per diffusion-factor component = LocalEvaluation::Elliptic +    */
/* SWIPDG::Inner + SWIPDG::BoundaryLHS, scattered into Q+1 CSR value arrays on one pattern; and the  */
/* BlockSWIPDG boundary / coupling assemblers (block-swipdg.hh:1136-1179, 1270-1326).                */
/* ---------------------------------------------------------------------------------------------- */
typedef struct hdd_mesh_s {
  int32_t elem_type;          /* HDD_SIMPLEX | HDD_CUBE | HDD_HEX */
  int32_t degree;             /* polynomial degree p of the DG space (0 or 1: P1 / Q1; HDD_HEX: 1..3) */
  int64_t n_local;            /* columns of the SoA arrays (owned + ghosts) */
  int64_t own_begin, own_end; /* elements whose rows are assembled */
  const double* coords;       /* device, layout of hdd_local_fill */
  const int32_t* neighbors;   /* device */
  const uint32_t* face_info;  /* device */
  /* optional vertex-indexed geometry (hdd_local_vertices; both or neither, device): when present, the 2d
   * P1 / Q1 stiffness kernels read each element's vertices through elem_vertices from vertex_coords and
   * the neighbour's off-face vertex through its vertex id, instead of the element-major coords (4 B per
   * element vertex instead of 16; the shared vertex rows stay cache resident).  coords stays required
   * (right-hand sides, products, 3d, halo geometry).  The two representations must describe the SAME
   * geometry: a caller that moves the mesh or fills ghost coordinates itself must update vertex_coords too,
   * or pass elem_vertices = vertex_coords = NULL (the sharded step does the latter with
   * HDD_SHARD_HALO_GEOMETRY, whose ghost coordinates arrive in coords only). */
  const int32_t* elem_vertices;  /* [nvpe][n_local] */
  const double* vertex_coords;   /* [n_vertices][dim] */
} hdd_mesh;

typedef struct {              /* one diffusion-factor component kappa_q (a Stuff::LocalizableFunction) */
  int32_t kind;               /* HDD_FN_* */
  int32_t order;              /* integration order of the function (Expression: integration_order) */
  double c;                   /* CONST value, SINUSOID offset a */
  double b, kx, ky;           /* SINUSOID: a + b*sin(kx*x + ky*y);
                                 COS_PRODUCT: a*cos(kx*x)*cos(ky*y) [*cos(b*z) in 3d when b != 0]
                                 (ESV2007 Testcase1Force, problems/ESV2007.hh:78) -- right-hand sides */
  const double* per_elem;     /* PER_ELEM: device [n_local] */
  /* FLATTOP: c + b * sum_k value_k phi(x; lx_k, ux_k, layer_x_k) phi(y; ly_k, uy_k, layer_y_k) -- the sum of
   * dune-stuff FlatTop functions the Spe10::Model1 channel is built from when channel_boundary_layer != 0
   * (problems/spe10.hh:139-148, 213-222): per coordinate 1 on [l + d, u - d], 0 outside [l - d, u + d] and
   * the C^1 cubic transitions (1 + t)^2 (1 - 2t), t = (x - (l + d)) / 2d in [-1, 0), and (1 - t)^2 (1 + 2t),
   * t = (x - (u - d)) / 2d in [0, 1) (layers d > 0).  `order` is the integration order the caller
   * assigns to the function (Stuff's order()).  2d meshes only. */
  const double* table;        /* FLATTOP: device [n_table][HDD_FLATTOP_REC] */
  int32_t n_table;            /* FLATTOP: number of boxes */
  int32_t pad1;
} hdd_scalar_fn;

typedef struct {              /* the (non-parametric) diffusion tensor A */
  int32_t kind;               /* HDD_TENSOR_* */
  int32_t pad;
  double c[6];                /* CONST: 2d a11 a12 a22; 3d a11 a12 a13 a22 a23 a33 */
  const double* per_elem;     /* ISO: device [n_local]; SYM: device [3 | 6][n_local] */
} hdd_tensor_fn;

typedef struct {
  double sigma_inner;         /* LocalEvaluation::SWIPDG::internal::inner_sigma(p)    (8 at p=1) */
  double sigma_boundary;      /* LocalEvaluation::SWIPDG::internal::boundary_sigma(p) (14 at p=1) */
  double beta;                /* LocalEvaluation::SWIPDG::internal::default_beta(d) = 1/(d-1) (swipdg.hh:168) */
  int32_t vol_order;          /* -1: the reference's integrand order (ord kappa + ord A + 2 max(p-1, 0)) */
  int32_t face_order;         /* -1: ord kappa + ord A + 2p */
} hdd_swipdg_params;

typedef struct {
  int64_t n_rows, n_cols, nnz;
  const int64_t* row_ptr;     /* device [n_rows+1] */
  const int32_t* col;         /* device [nnz] */
  const int64_t* elem_ptr;    /* device [n_owned+1]: first value of each owned element's row block */
} hdd_csr;

/* Device pattern build (the pattern of a p=3 3d mesh is ~4 bytes x 28672 per
 * element, too large to build on the host).  Step 1 writes d_elem_ptr [n_own+1] and returns the total
 * nnz in *nnz (host; synchronises `stream`; the kernel writes nnz into a mapped pinned word the context
 * allocates on its first call, so one stream at a time per context).  Step 2 writes d_row_ptr [nb*n_own+1] and d_col [nnz];
 * d_global_id [n_local] maps local to global element ids (NULL: local == global). */
int hdd_pattern_elem_ptr_device(hdd_ctx* ctx, const hdd_mesh* mesh, int32_t nb, int64_t* d_elem_ptr,
                                int64_t* nnz, void* stream);
int hdd_pattern_fill_device(hdd_ctx* ctx, const hdd_mesh* mesh, int32_t nb, const int64_t* d_global_id,
                            const int64_t* d_elem_ptr, int64_t* d_row_ptr, int32_t* d_col, void* stream);

/* Writes d_vals[q][0..nnz) for q < n_comp (each value exactly once, no atomics, no zero-fill needed).
 * Face terms are evaluated by the row owner on both sides of each face (owner-computes). */
int hdd_swipdg_assemble(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_scalar_fn* kappa, int32_t n_comp,
                        const hdd_tensor_fn* tensor, const hdd_swipdg_params* params, const hdd_csr* pattern,
                        double* const* d_vals, void* stream);

/* Same, restricted to the 64-element tiles d_tiles[0..n_tiles) (tile t = owned elements
 * [own_begin + 64t, own_begin + 64t + 64)): lets a sharded assembly run its interior tiles while the face
 * halo is in flight and the halo-dependent tiles afterwards.  Only the thread-per-element kernels
 * (P1 / Q1 with the reference integrand orders) take tile lists; others return HDD_ERR_UNSUPPORTED. */
int hdd_swipdg_assemble_tiles(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_scalar_fn* kappa, int32_t n_comp,
                              const hdd_tensor_fn* tensor, const hdd_swipdg_params* params, const hdd_csr* pattern,
                              double* const* d_vals, const int32_t* d_tiles, int64_t n_tiles, void* stream);

/* Same, restricted to the single owned elements own_begin + d_elems[0..n_elems) (one lane each, any order,
 * no duplicates): the fixup pass of a sharded step, which assembles every tile while the halo is in flight
 * (ghost rows stale) and then recomputes only the row blocks of elements with a ghost face neighbour.
 * Same kernel coverage as hdd_swipdg_assemble_tiles. */
int hdd_swipdg_assemble_elements(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_scalar_fn* kappa, int32_t n_comp,
                                 const hdd_tensor_fn* tensor, const hdd_swipdg_params* params,
                                 const hdd_csr* pattern, double* const* d_vals, const int32_t* d_elems,
                                 int64_t n_elems, void* stream);

/* SWIPDG right-hand side -- replaces the functionals of SWIPDG::init() (swipdg.hh:251-347):
 *   L2Volume(force) + DirichletBoundarySWIPDG(kappa, tensor, dirichlet) on Dirichlet faces
 *   + L2Face(neumann) on Neumann faces, each of force / dirichlet / neumann nullable (absent = zero).
 * Writes d_rhs[k*nb + i] for every owned element k (local order) and basis function i; one call per
 * affine component of the right-hand side (the caller pairs kappa / dirichlet components as swipdg.hh
 * does).  Integration orders: ord(f) + p; Neumann ord(g_N) + p; Dirichlet max(ord(g_D) + p,
 * ord(kappa) + ord(A) + p - 1 + ord(g_D)).  2d meshes with Dirichlet or Neumann data: two launches (volume
 * kernel, then a face kernel over the boundary elements the first one listed) on a list the context holds
 * (16 B per owned element, allocated on the first call of a size class: warm a context up before hipGraph
 * capture).  Eager calls of one context on different streams are ordered behind each other by the library (an
 * event on the previous call's stream).  A CAPTURED call is not: the replays of a graph that captured an
 * hdd_swipdg_rhs call of context C must not run concurrently with eager hdd_swipdg_rhs calls of C or with replays
 * of another such graph of C (they share C's list); use a separate context per concurrent graph / stream. */
int hdd_swipdg_rhs(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_scalar_fn* force, const hdd_scalar_fn* kappa,
                   const hdd_tensor_fn* tensor, const hdd_scalar_fn* dirichlet, const hdd_scalar_fn* neumann,
                   const hdd_swipdg_params* params, double* d_rhs, void* stream);

/* Products of SWIPDG::init() (swipdg.hh:358-508; over_integrate = 2) -- BlockSWIPDG's local products
 * (block-swipdg.hh:392-548) are the same on the subdomain's elements:
 *   HDD_PRODUCT_L2, _H1_SEMI, _ELLIPTIC (kappa, tensor), _BOUNDARY_L2: element-local blocks; pattern =
 *   hdd_dg_pattern_fill with n_faces = 0 (row length nb);
 *   HDD_PRODUCT_PENALTY (kappa, tensor): the SWIPDG penalty terms sigma kappa^- kappa^+ gamma / |F|^beta on
 *   inner faces and the boundary penalty on Dirichlet faces; pattern = the SWIPDG pattern.
 * Writes d_vals[0..nnz) (every entry once).
 * Pattern check: the element-local kinds return HDD_ERR_INVALID unless pattern->nnz == nb * nb * owned elements
 * (a SWIPDG pattern has the right row count but another layout); the penalty returns HDD_ERR_INVALID when
 * pattern->nnz < nb * nb * owned elements.  Beyond that the host cannot verify a penalty pattern (its blocks per row
 * are in the device arrays): the caller must pass the SWIPDG pattern of this mesh -- the kernel writes
 * nb * (1 + interior faces) values per row, which a volume pattern's value array does not hold. */
enum { HDD_PRODUCT_L2 = 0, HDD_PRODUCT_H1_SEMI = 1, HDD_PRODUCT_ELLIPTIC = 2, HDD_PRODUCT_BOUNDARY_L2 = 3,
       HDD_PRODUCT_PENALTY = 4 };
int hdd_product_assemble(hdd_ctx* ctx, const hdd_mesh* mesh, int32_t product, const hdd_scalar_fn* kappa,
                         const hdd_tensor_fn* tensor, const hdd_swipdg_params* params, const hdd_csr* pattern,
                         double* d_vals, void* stream);

/* theta-lincomb of affine components on a shared pattern -- replaces
 * AffinelyDecomposedContainer::freeze_parameter(mu) as used by ContainerBasedDefault::uncached_solve
 * (base.hh:338-341, 357-361):  out[s][k] = sum_q theta[s*n_comp+q] * d_vals[q][k]  (theta on host) */
int hdd_affine_lincomb(hdd_ctx* ctx, int64_t nnz, const double* const* d_vals, int32_t n_comp,
                       const double* theta, int32_t n_samples, double* d_out, int64_t out_stride, void* stream);

/* ---------------------------------------------------------------------------------------------- */
/* halo records (face-coupling ghosts of a sharded BlockSWIPDG) -- SoA gather / scatter of element    */
/* columns; the transport itself is RCCL send/recv (torch.distributed) between the two calls.         */
/* ---------------------------------------------------------------------------------------------- */
/* buf[(r)*n + i] = arrays[a][row(a,r)*ld + idx[i]] for the concatenated rows of all arrays */
int hdd_soa_gather(hdd_ctx* ctx, const double* const* arrays, const int32_t* rows, int32_t n_arrays, int64_t ld,
                   const int32_t* d_idx, int64_t n, double* d_buf, void* stream);
/* arrays[a][row*ld + dst_offset + i] = buf[r*n + i] */
int hdd_soa_scatter(hdd_ctx* ctx, double* const* arrays, const int32_t* rows, int32_t n_arrays, int64_t ld,
                    int64_t dst_offset, int64_t n, const double* d_buf, void* stream);

/* ---------------------------------------------------------------------------------------------- */
/* block operators -- replaces BlockSWIPDG::get_local_operator(ss) / get_coupling_operator(ss, nn)   */
/* (block-swipdg.hh:625-676): in the subdomain-major numbering they are the diagonal / off-diagonal   */
/* blocks of the global matrix, extracted through a value map built once from the pattern.            */
/* ---------------------------------------------------------------------------------------------- */
/* rows of subdomain ss, columns of subdomain nn (ss == nn: local operator), local numbering on both
 * sides.  Call with out_col == NULL to get *nnz; out_row_ptr [rows+1], out_col / out_src [nnz]
 * (out_src = index of each extracted value in the global value array).  Host arrays. */
int hdd_block_operator_map(const hdd_grid* g, int32_t ss, int32_t nn, const int64_t* row_ptr, const int32_t* col,
                           int64_t* out_row_ptr, int32_t* out_col, int64_t* out_src, int64_t* nnz);
/* d_out[k] = d_vals[d_src[k]] for k < n (device arrays) */
int hdd_gather_values(hdd_ctx* ctx, const double* d_vals, const int64_t* d_src, int64_t n, double* d_out, void* stream);
/* The same on the device, from the device pattern: rows [row_begin, row_end) of `pattern` restricted to the
 * columns [col_begin, col_end) (operator (ss, nn): rows / columns of the element ranges of ss / nn times nb,
 * hdd_grid_subdomain_range), renumbered col - col_begin.  Writes d_out_row_ptr [rows+1] always; d_out_col /
 * d_out_src [nnz] when d_out_col != NULL (d_out_src nullable); *nnz (host) when nnz != NULL, which
 * synchronises `stream` -- call once with d_out_col == NULL and nnz to size the arrays, or pass the known
 * nnz (nb^2 x the ss/nn element-face pairs, plus nb^2 |ss| for ss == nn) and stay asynchronous. */
int hdd_block_operator_map_device(hdd_ctx* ctx, const hdd_csr* pattern, int64_t row_begin, int64_t row_end,
                                  int64_t col_begin, int64_t col_end, int64_t* d_out_row_ptr, int32_t* d_out_col,
                                  int64_t* d_out_src, int64_t* nnz, void* stream);
/* the operator's values of n_comp value arrays on `pattern` (d_out_row_ptr from the map call): no index map */
int hdd_block_operator_values_device(hdd_ctx* ctx, const hdd_csr* pattern, int64_t row_begin, int64_t row_end,
                                     int64_t col_begin, int64_t col_end, const int64_t* d_out_row_ptr,
                                     const double* const* d_vals, int32_t n_comp, double* const* d_out, void* stream);

/* Batched: n_ops operators of one pattern in four launches (count, one scan over all, bases, fill) -- e.g.
 * every get_local_operator / get_coupling_operator of a BlockSWIPDG at once.  Outputs are concatenated:
 * operator k's row pointer [rows_k + 1] (operator-relative, starting at 0) is at d_out_row_ptr + row_off_k,
 * row_off_k = sum_{j<k} (rows_j + 1); its local columns / source positions at d_out_col / d_out_src +
 * nnz_off[k] (either may be NULL), nnz_off[k+1] = nnz_off[k] + nnz_k + (nnz_k & 1): every operator starts
 * 16-byte aligned in the value arrays (one padding entry after an odd count, left unwritten).  nnz_off (host
 * [n_ops + 1], nnz_off[n_ops] = the padded total) is returned when non-NULL, which synchronises `stream`; a
 * caller that knows the counts (from the mesh: nb^2 x face pairs, + nb^2 |ss| on the diagonal) passes NULL
 * and stays asynchronous.  sum_k (rows_k + 1) < 2^31. */
typedef struct {
  int64_t row_begin, row_end, col_begin, col_end;
} hdd_block_range;
int hdd_block_operators_map_device(hdd_ctx* ctx, const hdd_csr* pattern, int32_t n_ops, const hdd_block_range* ops,
                                   int64_t* d_out_row_ptr, int32_t* d_out_col, int64_t* d_out_src, int64_t* nnz_off,
                                   void* stream);
/* the operators' values of n_comp value arrays (concatenated like the columns; nnz_off host [n_ops + 1]) */
int hdd_block_operators_values_device(hdd_ctx* ctx, const hdd_csr* pattern, int32_t n_ops, const hdd_block_range* ops,
                                      const int64_t* nnz_off, const int64_t* d_out_row_ptr, const double* const* d_vals,
                                      int32_t n_comp, double* const* d_out, void* stream);

/* ---------------------------------------------------------------------------------------------- */
/* operator application -- what the reference's consumers do with the assembled containers: pyMOR's  */
/* apply / apply2 on the LinearAffinelyDecomposedContainerBased operator of get_operator() and on the */
/* products (base.hh:45, 260-264), LRBMS on every get_local_operator(ss) / get_coupling_operator(ss,  */
/* nn) (block-swipdg.hh:625-676), the applies inside uncached_solve's solver (base.hh:327-367).       */
/* Additive to ABI 8.                                                                               */
/* ---------------------------------------------------------------------------------------------- */
#define HDD_MAX_VEC 8
/* y[v][r - row_begin] = sum_q theta[q] * sum_{k in row r, col_begin <= col[k] < col_end}
 *                       d_vals[q][k] * x[v][col[k] - col_begin]
 * for r in [row_begin, row_end), v < n_vec.  y is overwritten and must not overlap x.  x is [n_vec][ldx]
 * (ldx >= col_end - col_begin), y is [n_vec][ldy] (ldy >= row_end - row_begin), both device.
 * d_vals: host array of n_comp (1..HDD_MAX_COMP) device value arrays on `pattern`; theta: host [n_comp], NULL = all
 * ones -- sum_q theta_q A_q is applied without ever being written (no hdd_affine_lincomb, no room for A(mu)).
 * range: NULL = the whole matrix; else the operator (ss, nn) of a BlockSWIPDG is rows / columns of the element
 * ranges of ss / nn times nb (hdd_grid_subdomain_range), applied in place, no extraction.  Entries outside the
 * column range are skipped, not multiplied by zero: x is never read outside [0, col_end - col_begin) and a NaN in
 * a skipped value does not reach y.
 * mesh: NULL, or the mesh whose SWIPDG face pattern `pattern` is (hdd_pattern_fill / hdd_dg_pattern_fill with the
 * mesh's faces / hdd_pattern_fill_device on this mesh) -- BY PASSING mesh THE CALLER ASSERTS THIS; the library
 * cannot check it.  With a 2d HDD_SIMPLEX / HDD_CUBE mesh (degree <= 1), pattern->elem_ptr, n_cols == nb * n_local
 * (local == global numbering: the whole-grid view), a range whose four bounds are multiples of nb, 16-byte aligned
 * value arrays and fewer than 2^29 columns in range, the call takes the tile kernel, which derives every column from
 * mesh->neighbors and reads neither col nor row_ptr (8 B per nonzero).  Everything else -- mesh == NULL, hexahedra,
 * volume-only product patterns (pass mesh = NULL for them: their pattern is not the face pattern), extracted block
 * operators, renumbered columns, a range that is not nb-aligned -- takes the plain CSR kernel on row_ptr / col with the
 * same semantics.  hdd_last_apply_kernel() names the path taken.
 * Asynchronous on `stream`; allocates nothing, synchronises nothing, uses no atomics: results are bit-identical
 * from call to call.  Every argument check precedes the first device call: HDD_ERR_INVALID for a null ctx /
 * pattern / d_vals / d_vals[q] / d_x / d_y, n_comp outside 1..HDD_MAX_COMP, n_vec outside 1..HDD_MAX_VEC, ldx / ldy
 * too small, a range outside the matrix, a mesh that does not match the pattern's rows. */
int hdd_operator_apply(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
                       int32_t n_comp, const double* theta, const hdd_block_range* range, const double* d_x,
                       int64_t ldx, double* d_y, int64_t ldy, int32_t n_vec, void* stream);
/* d_out[i*n_u + j] = v_i^T (sum_q theta_q A_q) u_j on the same (restricted) operator; i < n_v, j < n_u, both in
 * 1..HDD_MAX_VEC: pyMOR's apply2, a reduced-basis projection V^T A_q V, a product's Gramian.  d_v is [n_v][ldv]
 * (ldv >= rows), d_u [n_u][ldu] (ldu >= columns), d_work the caller's [n_u][ldw] scratch, ldw >= rows; d_out device
 * [n_v*n_u].  It is hdd_operator_apply into d_work followed by a two-stage reduction in a fixed order (per-block
 * partial sums in a buffer the context owns since its creation, then the blocks in order): same rules as above, and
 * one stream at a time per context. */
int hdd_operator_apply2(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
                        int32_t n_comp, const double* theta, const hdd_block_range* range, const double* d_v,
                        int64_t ldv, int32_t n_v, const double* d_u, int64_t ldu, int32_t n_u, double* d_work,
                        int64_t ldw, double* d_out, void* stream);
/* the kernel the last hdd_operator_apply / _apply2 / _project of this thread launched ("" if none), like
 * hdd_last_tile_kernel: "apply_tile_kernel<NB, NF, NV>" or "apply_csr_kernel<G, NV>" ("project_tile_kernel<NB, NF>",
 * "project_csr_kernel<G>") */
const char* hdd_last_apply_kernel(void);

/* ---------------------------------------------------------------------------------------------- */
/* reduced-basis projection -- every affine component onto a basis in one pass over the values:     */
/* G_q = V^T A_q U, the reduced right-hand sides V^T b_q, a product's Gramian.  Additive to ABI 8.   */
/* ---------------------------------------------------------------------------------------------- */
#define HDD_MAX_BASIS 64
/* doubles of workspace; a function of its arguments alone; 0 for arguments the call would reject.  The calls below
 * leave at most 512 partial sums per entry there: 512 * n_comp * n_v * n_u doubles -- 8 MiB for two components on a
 * 32 x 32 basis, 128 MiB at n_comp = 8, 64 x 64. */
int64_t hdd_operator_project_workspace(int32_t n_comp, int32_t n_v, int32_t n_u);
/* d_out[(q*n_v + i)*n_u + j] = v_i^T A_q u_j on the (restricted) operator; q < n_comp, i < n_v, j < n_u, n_v and n_u
 * in 1..HDD_MAX_BASIS.  No theta: the components come out separately, A(mu) reduced is a host lincomb of small
 * matrices.  mesh / pattern / d_vals / range follow hdd_operator_apply's rules: the operator (ss, nn) of a BlockSWIPDG
 * is projected in place through `range` (v in ss's numbering, u in nn's); entries outside the column range are
 * skipped, not multiplied by zero, and neither they nor the padding behind ldv / ldu are read.  d_v is [n_v][ldv]
 * (ldv >= rows), d_u [n_u][ldu] (ldu >= columns), d_work the caller's n_work >=
 * hdd_operator_project_workspace(n_comp, n_v, n_u) doubles, d_out device [n_comp*n_v*n_u].
 * W = A_q U is never written: a wave forms it for a panel of 16 u-vectors on its rows and contracts it at once with
 * the same rows of V on the f64 matrix cores; every workgroup leaves its share in d_work and a second kernel adds
 * the workgroups in order.  The mesh of a 2d P1 / Q1 whole-grid face pattern with an nb-aligned range selects the
 * tile kernel (hdd_last_apply_kernel(): "project_tile_kernel<3, 3>" / "<4, 4>"), everything else the CSR kernel
 * ("project_csr_kernel<8>" / "<64>"), as for hdd_operator_apply.
 * Asynchronous on `stream`; allocates nothing, synchronises nothing, uses no atomics: bit-identical from call to call.
 * On a given path entry (q, i, j) is a function of A_q, v_i, u_j and the range alone -- not of n_v, n_u, the other
 * vectors or the position of v_i / u_j in the call: a basis extended by one vector needs only the new row and column,
 * which are bit for bit those of the full re-projection.
 * Every argument check precedes the first device call: HDD_ERR_INVALID for a null pointer, n_comp outside
 * 1..HDD_MAX_COMP, n_v / n_u outside 1..HDD_MAX_BASIS, ldv / ldu too small, n_work below the workspace function's
 * value, a range outside the matrix, a mesh that does not match the pattern's rows. */
int hdd_operator_project(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
                         int32_t n_comp, const hdd_block_range* range, const double* d_v, int64_t ldv, int32_t n_v,
                         const double* d_u, int64_t ldu, int32_t n_u, double* d_work, int64_t n_work, double* d_out,
                         void* stream);
/* d_out[i*n_w + j] = v_i . w_j over n entries, n_v and n_w in 1..HDD_MAX_BASIS: reduced right-hand sides V^T b_q,
 * functionals, a Euclidean Gramian.  d_v is [n_v][ldv], d_w [n_w][ldw] (ldv, ldw >= n), d_work the caller's n_work >=
 * hdd_operator_project_workspace(1, n_v, n_w) doubles.  The same two stages and the same guarantees as
 * hdd_operator_project. */
int hdd_vectors_inner(hdd_ctx* ctx, const double* d_v, int64_t ldv, int32_t n_v, const double* d_w, int64_t ldw,
                      int32_t n_w, int64_t n, double* d_work, int64_t n_work, double* d_out, void* stream);

/* ---------------------------------------------------------------------------------------------- */
/* solve -- the apply_inverse of ContainerBasedDefault::uncached_solve (base.hh:327-367) on the      */
/* theta-fused operator: (block-)Jacobi preconditioned conjugate gradients, on the device between    */
/* two looks of the host.  Additive to ABI 8.                                                        */
/* ---------------------------------------------------------------------------------------------- */
enum { HDD_PRECOND_NONE = 0, HDD_PRECOND_BLOCK_JACOBI = 1 };
enum { HDD_SOLVE_CONVERGED = 0, HDD_SOLVE_MAX_ITER = 1, HDD_SOLVE_BREAKDOWN = 2 };
enum { HDD_SOLVE_X0 = 1 };            /* flags: d_x holds the initial guess (default: x0 = 0, d_x need not be set) */
typedef struct {
  double rtol, atol;                  /* stop when ||r||_2 <= max(rtol * ||b||_2, atol), r the recurrence residual */
  int32_t max_iter;
  int32_t check_every;                /* iterations enqueued between two looks of the host; 0 = default (32) */
  int32_t precond;                    /* HDD_PRECOND_* */
  int32_t block_size;                 /* block-Jacobi block: 0 = nb of the mesh (needs mesh); else 1..8 */
  int32_t flags, pad;
} hdd_solve_options;
typedef struct { int32_t status, iterations; double residual, rhs_norm; } hdd_solve_info;

/* doubles of workspace hdd_operator_solve needs for `rows` rows and blocks of block_size (1..8) rows; with
 * block_size 0 (the mesh's nb, which this function cannot know) enough for every block size.  0 for a negative
 * rows or a block_size outside 0..8.  The solve checks n_work against the block size it resolves, so block_size 0
 * on a P1 mesh needs what block_size 3 needs. */
int64_t hdd_operator_solve_workspace(int64_t rows, int32_t block_size);
/* Solves (sum_q theta[q] A_q) x = b by preconditioned conjugate gradients.  mesh, pattern, d_vals, n_comp, theta are
 * hdd_operator_apply's, with the same checks and the same dispatch (the tile kernel where apply takes it, the CSR
 * kernel otherwise); range is NULL (the whole matrix, which must be square) or a square diagonal range (row_begin ==
 * col_begin, row_end == col_end): the local solve on a BlockSWIPDG's get_local_operator(ss), in place.  d_b, d_x:
 * device [rows], one right-hand side per call (several: hdd_operator_solve_batched below).  d_x is overwritten; with
 * HDD_SOLVE_X0 it is read first as the initial guess.
 * THE MATRIX MUST BE SYMMETRIC POSITIVE DEFINITE -- BY CALLING THE CALLER ASSERTS THIS; the library cannot check it.
 * The SWIPDG matrix with the reference's penalties (8 / 14) is positive definite on near-square elements with a
 * diffusion that is constant per element, but INDEFINITE on stretched elements under a high-contrast diffusion and
 * for the strongly varying smooth diffusion of OS2014 (tables in DESIGN.md 4.7); HDD_SOLVE_BREAKDOWN is what a
 * violated assertion may produce (it may also end in MAX_ITER).
 * Preconditioner: HDD_PRECOND_BLOCK_JACOBI inverts the diagonal blocks of block_size rows (0: nb of the mesh, one
 * block per element; the bounds of the range, or n_rows, must be multiples of it) once per call into the workspace;
 * a block with a non-positive pivot gives HDD_SOLVE_BREAKDOWN before the first iteration.
 * Iteration: three launches (q = A p with p . q in its epilogue; x, r, z and their dot products; the new direction),
 * no atomics, every sum two-stage in a fixed order: x, iterations and residual are bit-identical from call to call
 * and do not depend on check_every.  Every launch of an iteration reads a stop word first, which the device sets on
 * convergence (||r|| <= max(rtol ||b||, atol), r the recurrence residual) or breakdown (p . Ap <= 0, r . z <= 0, a
 * non-finite scalar): the host enqueues min(check_every, remaining) iterations, then copies 64 bytes of state back
 * and SYNCHRONISES `stream` -- at every look, and before returning.  info: status HDD_SOLVE_*, the iterations done,
 * the recurrence ||r||_2 and ||b||_2.  With ||b|| = 0: x = 0, converged, 0 iterations (a right-hand side that holds a
 * NaN is not that: it is a breakdown before the first iteration).  On breakdown x is the last
 * iterate before it.  d_history: NULL or device [max_iter + 1], entry k = ||r_k||_2 for k <= iterations.
 * Allocates nothing: d_work (n_work >= hdd_operator_solve_workspace doubles, 16-byte aligned for the 16-byte access
 * paths) holds every vector, the inverse blocks and the state; the context owns the pinned bytes the state is read
 * back into since its creation.  One stream at a time per context.
 * Returns HDD_OK for all three statuses; HDD_ERR_INVALID (every argument check precedes the first device call) for a
 * null ctx / pattern / d_vals / d_b / d_x / opt / d_work / info, what hdd_operator_apply rejects, a range that is
 * not square and diagonal, max_iter < 0, rtol / atol negative or NaN, check_every < 0, an unknown precond, block_size
 * outside 0..8, block_size 0 without a mesh of nb <= 8, bounds that are no multiples of the block size, n_work too
 * small; HDD_ERR_HIP for a HIP failure. */
int hdd_operator_solve(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
                       int32_t n_comp, const double* theta, const hdd_block_range* range, const double* d_b,
                       double* d_x, const hdd_solve_options* opt, double* d_work, int64_t n_work, double* d_history,
                       hdd_solve_info* info, void* stream);
/* the kernels of one iteration of this thread's last hdd_operator_solve ("" if none), e.g.
 * "apply_tile_kernel<3, 3, 1, dot> + cg_update<3> + cg_direction" */
const char* hdd_last_solve_kernels(void);

/* Several right-hand sides against one matrix per call: pyMOR's apply_inverse on a VectorArray (the Riesz
 * representatives product^-1 R of a reductor), the local corrections of LRBMS on one get_local_operator(ss).
 * Additive to ABI 8.
 * doubles of workspace hdd_operator_solve_batched needs: the vectors and partial sums per right-hand side, the
 * inverse blocks once.  block_size as in hdd_operator_solve_workspace; 0 for a negative rows, a block_size outside
 * 0..8 or n_rhs outside 1..HDD_MAX_VEC. */
int64_t hdd_operator_solve_batched_workspace(int64_t rows, int32_t block_size, int32_t n_rhs);
/* hdd_operator_solve for n_rhs (1..HDD_MAX_VEC) right-hand sides: d_b is [n_rhs][ldb], d_x [n_rhs][ldx] (ldb, ldx >=
 * rows; d_x must not overlap d_b), d_history NULL or [n_rhs][ldh] with ldh >= max_iter + 1, info host [n_rhs].  The
 * operator arguments, the range rule, the dispatch and the options are hdd_operator_solve's; one hdd_solve_options
 * holds for every column, and with HDD_SOLVE_X0 every column of d_x is read as that column's initial guess.
 * Column j ends with exactly the x, iterations, residual, rhs_norm, status and history that hdd_operator_solve gives
 * for (b_j, x0_j) with the same options -- the doubles bit for bit, whatever the other columns hold and whatever
 * check_every is.  A column that is done (converged, broken down, zero right-hand side) is frozen: later iterations
 * do not touch its x.  A NaN or a breakdown (p . Ap <= 0) stays in its own column; a diagonal block that is not
 * positive definite breaks every column down before the first iteration; a zero column gives x_j = 0, converged, 0
 * iterations.  Returns HDD_OK for every mix of per-column statuses.
 * The columns run in groups of four (the multi-vector pass of hdd_operator_apply): per group and iteration the same
 * three launches as hdd_operator_solve, which read the value arrays and the inverse blocks once for the group.  Each
 * column keeps its own sums on the single solve's grids, its own 64-byte state and stop word; a group has a stop
 * word of its own (the iteration at which its last live column ended).  At every look the host copies all states
 * back in one copy and SYNCHRONISES `stream`; it stops when every column is done or max_iter is reached.
 * Allocates nothing, no atomics, one stream at a time per context.  HDD_ERR_INVALID (every argument check precedes
 * the first device call) for what hdd_operator_solve rejects, n_rhs outside 1..HDD_MAX_VEC, ldb or ldx < rows, a
 * history with ldh < max_iter + 1, n_work below hdd_operator_solve_batched_workspace, a null info.
 * hdd_last_solve_kernels() afterwards names the batched kernels with the vector count of their instantiation (4, not
 * n_rhs): "apply_tile_kernel<3, 3, 4, dot> + cg_update<3, 4> + cg_direction<4>" (without a preconditioner
 * "cg_update<3, none, 4>"). */
int hdd_operator_solve_batched(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
                               int32_t n_comp, const double* theta, const hdd_block_range* range, const double* d_b,
                               int64_t ldb, double* d_x, int64_t ldx, int32_t n_rhs, const hdd_solve_options* opt,
                               double* d_work, int64_t n_work, double* d_history, int64_t ldh, hdd_solve_info* info,
                               void* stream);

/* The same affine components at several parameters per call: column j has a theta of its own, theta_j = theta + j *
 * ldt (host [n][ldt], ldt >= n_comp; NULL = all ones for every column).  This is the multi-query workload -- the
 * snapshots and estimator residuals of a parametric study or a greedy loop are A(mu_j) = sum_q theta_q(mu_j) A_q on
 * one pattern with one set of value arrays, which are read once per group of four columns instead of once per
 * parameter.  Additive to ABI 8.
 *
 * hdd_operator_apply_multi: y_j = (sum_q theta_j[q] A_q) x_j, j < n_vec.  Every other argument, check, the range rule
 * and "allocates nothing, no atomics" are hdd_operator_apply's.
 * CONTRACT: column j is bit for bit what hdd_operator_apply gives for (theta_j, x_j) on the same path -- the matrix
 * entry of column j is formed as there (theta_j[0] a_0, then one FMA per further component), then one FMA into the
 * column's sum.  With theta NULL the call equals hdd_operator_apply's multi-vector result bit for bit.
 * Dispatch: the tile kernel stages one LDS image per component, so it takes what hdd_operator_apply's tile path takes
 * only for P1 with n_comp <= 3 and Q1 with n_comp == 1 (the images of a wave within the 64 KB of LDS a launch gets by
 * default); everything else takes the CSR kernel (every n_comp <= HDD_MAX_COMP; the pattern then needs row_ptr / col)
 * and is bit for bit hdd_operator_apply with mesh == NULL.  hdd_last_apply_kernel() names
 * "apply_tile_multi_kernel<NB, NF, NV>" or "apply_csr_multi_kernel<G, NV>" (NV = 4 whatever n_vec is).
 * HDD_ERR_INVALID also for a non-null theta with ldt < n_comp. */
int hdd_operator_apply_multi(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
                             int32_t n_comp, const double* theta, int64_t ldt, const hdd_block_range* range,
                             const double* d_x, int64_t ldx, double* d_y, int64_t ldy, int32_t n_vec, void* stream);
/* doubles of workspace hdd_operator_solve_multi needs: hdd_operator_solve_batched_workspace with the inverse blocks
 * n_rhs times (every column's preconditioner is that of its own theta_j).  0 for the same bad arguments. */
int64_t hdd_operator_solve_multi_workspace(int64_t rows, int32_t block_size, int32_t n_rhs);
/* hdd_operator_solve_batched with a theta per column: solves (sum_q theta_j[q] A_q) x_j = b_j for j < n_rhs in one
 * call.  Every argument but theta / ldt, the range rule, the options, info, history, HDD_SOLVE_X0, the looks of the
 * host, "allocates nothing" and "one stream at a time per context" are hdd_operator_solve_batched's; the dispatch is
 * hdd_operator_apply_multi's.
 * CONTRACT: column j ends with exactly the x, iterations, residual, rhs_norm, status and history that
 * hdd_operator_solve gives for (theta_j, b_j, x0_j) with the same options on the same path -- the doubles bit for
 * bit, whatever the other columns and their thetas are and whatever check_every is.  With theta NULL the call equals
 * hdd_operator_solve_batched bit for bit.
 * EVERY A(theta_j) MUST BE SYMMETRIC POSITIVE DEFINITE -- by calling the caller asserts this PER theta_j (a sum of
 * components that is definite at one parameter need not be at another: DESIGN.md 4.7).
 * Per-column breakdown: the inverse diagonal blocks are computed per column at theta_j into that column's slice of
 * the workspace, with a count of blocks that are not positive definite per column.  Such a block at theta_j gives
 * column j alone HDD_SOLVE_BREAKDOWN with 0 iterations, as the single solve at theta_j reports it; the other columns
 * iterate on, frozen columns are not touched, and the call returns HDD_OK.  With HDD_SOLVE_X0 the initial residual is
 * b_j - A(theta_j) x0_j by hdd_operator_apply_multi.  The columns run in groups of four.
 * HDD_ERR_INVALID (every argument check precedes the first device call) for what hdd_operator_solve_batched rejects,
 * a non-null theta with ldt < n_comp, n_work below hdd_operator_solve_multi_workspace.
 * hdd_last_solve_kernels(): "apply_tile_multi_kernel<3, 3, 4, dot> + cg_update<3, 4, own> + cg_direction<4>" (without
 * a preconditioner "cg_update<3, none, 4>"). */
int hdd_operator_solve_multi(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
                             int32_t n_comp, const double* theta, int64_t ldt, const hdd_block_range* range,
                             const double* d_b, int64_t ldb, double* d_x, int64_t ldx, int32_t n_rhs,
                             const hdd_solve_options* opt, double* d_work, int64_t n_work, double* d_history,
                             int64_t ldh, hdd_solve_info* info, void* stream);

/* Every subdomain at once: the block-diagonal part of sum_q theta[q] A_q with respect to the segments of a partition
 * of a row interval -- the local corrections, local Riesz representatives and enrichment solves of LRBMS, which solve
 * on get_local_operator(ss) for ALL ss, and the non-overlapping Schwarz preconditioner sum_s R_s^T A_ss^-1 R_s.  The
 * batch runs over row segments instead of columns.  Additive to ABI 8.
 *
 * bounds: host [n_blocks + 1], strictly ascending, inside the square part of the matrix; segment s is rows = columns
 * [bounds[s], bounds[s + 1]).  The bounds are rows, not subdomain ids; a segment may be several subdomains, and the
 * interval need neither begin at 0 nor end at n_rows.  The vectors (d_b, d_x; d_x, d_y of the apply) have bounds[n_blocks] -
 * bounds[0] entries, segment s at bounds[s] - bounds[0].  An entry whose column lies in another segment is skipped,
 * not multiplied by zero, as a range skips it.  The operator arguments, their checks and the dispatch are
 * hdd_operator_apply's per segment: the tile kernel where the call on every segment's range would take it (so every
 * bound a multiple of nb), the CSR kernel otherwise.
 *
 * hdd_operator_apply_blocks: y_s = A_ss x_s for every segment in one launch, one vector.  CONTRACT: segment s has the
 * bits of hdd_operator_apply on the range (bounds[s], bounds[s + 1], bounds[s], bounds[s + 1]) on the same path.
 * Allocates nothing (the segment table goes through buffers the context owns since its creation), no atomics, one
 * stream at a time per context.  hdd_last_apply_kernel(): "apply_tile_blocks_kernel<3, 3>", "apply_csr_blocks_kernel<8>". */
#define HDD_MAX_SOLVE_BLOCKS 4096
int hdd_operator_apply_blocks(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
                              int32_t n_comp, const double* theta, int32_t n_blocks, const int64_t* bounds,
                              const double* d_x, double* d_y, void* stream);
/* doubles of workspace hdd_operator_solve_blocks needs: a function of (rows, block_size, n_blocks) alone, rows =
 * bounds[n_blocks] - bounds[0] -- p, q, r, z and the packed inverse blocks of the interval, per segment a 64-byte
 * state and a 64-byte table entry, and the partial sums of all segments together, bounded by rows / 4 + n_blocks (the
 * workgroups of the apply) and four times rows / (256 block_size) + n_blocks (those of the update).  block_size as in
 * hdd_operator_solve_workspace; 0 for a negative rows, a block_size outside 0..8 or n_blocks outside
 * 1..HDD_MAX_SOLVE_BLOCKS. */
int64_t hdd_operator_solve_blocks_workspace(int64_t rows, int32_t block_size, int32_t n_blocks);
/* Solves A_ss x_s = b_s for every segment s in one call.  One hdd_solve_options holds for all segments (options,
 * HDD_SOLVE_X0 -- segment s of d_x is that segment's guess --, block-Jacobi with block_size 0..8 and "no
 * preconditioner" are hdd_operator_solve's); rtol is relative to each segment's own ||b_s||.  d_history: NULL or device
 * [n_blocks][ldh], ldh >= max_iter + 1; info: host [n_blocks].  EVERY A_ss MUST BE SYMMETRIC POSITIVE DEFINITE
 * (principal blocks of a definite matrix are).
 * CONTRACT: segment s ends with exactly the x_s, iterations, residual, rhs_norm, status and history that
 * hdd_operator_solve gives with the range (bounds[s], bounds[s + 1], bounds[s], bounds[s + 1]) on (b_s, x0_s) with the
 * same options on the same path -- the doubles bit for bit, whatever the other segments hold and whatever check_every
 * is.  Every segment runs on the grids its single solve has (virtual grids inside the launches), so every sum keeps
 * its order.
 * A segment that is done (converged, broken down, zero right-hand side) is frozen: no later launch touches its x.  A
 * NaN, a p . Ap <= 0, a zero b_s (x_s = 0, converged, 0 iterations; only that segment of x is cleared) and a diagonal
 * block that is not positive definite (breakdown before the first iteration: the count is kept per segment) stay
 * with their own segment.  Returns HDD_OK for every mix of statuses.
 * One iteration of the whole call is three launches, whatever n_blocks is; every launch reads the call's stop word
 * (the iteration at which the last live segment ended), then its segment's.  A look of the host renews and reads the
 * call's stop word and SYNCHRONISES `stream`; the per-segment states are read once, at the end.  Allocates nothing, no
 * atomics, one stream at a time per context; the segment table is one copy into the workspace per call.
 * HDD_ERR_INVALID (every argument check precedes the first device call) for what hdd_operator_solve rejects, n_blocks
 * outside 1..HDD_MAX_SOLVE_BLOCKS, null bounds, bounds not strictly ascending or outside the matrix, a bound that is no
 * multiple of the resolved block size, ldh < max_iter + 1 with a history, n_work below
 * hdd_operator_solve_blocks_workspace, a null info.
 * hdd_last_solve_kernels(): "apply_tile_blocks_kernel<3, 3, dot> + cg_update_blocks<3> + cg_direction_blocks"
 * ("apply_csr_blocks_kernel<8, dot>" on the CSR path, "cg_update_blocks<3, none>" without a preconditioner). */
int hdd_operator_solve_blocks(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
                              int32_t n_comp, const double* theta, int32_t n_blocks, const int64_t* bounds,
                              const double* d_b, double* d_x, const hdd_solve_options* opt, double* d_work,
                              int64_t n_work, double* d_history, int64_t ldh, hdd_solve_info* info, void* stream);

/* ---------------------------------------------------------------------------------------------- */
/* a-posteriori error estimator -- Estimators::SWIPDG (estimators/swipdg.hh), which the reference's  */
/* study calls right after every solve (test/linearelliptic-swipdg.hh:238-241, 302-315): the ESV2007   */
/* estimator of a P1 SWIPDG vector, on the device where the solve left it.  Additive to ABI 8.        */
/* ---------------------------------------------------------------------------------------------- */
/* Scope: 2d HDD_SIMPLEX meshes, degree 1; the whole-grid view (own_begin == 0, own_end == n_local, no ghosts: a
 * vertex patch needs every element around the vertex); every boundary face Dirichlet with g_D = 0 (the reference's
 * Oswald operator assumes it); diffusion factor components HDD_FN_CONST or HDD_FN_PER_ELEM, combined as kappa_T(theta)
 * = sum_q theta_q kappa_q,T; any tensor kind; a force of any hdd_scalar_fn kind (NULL: f = 0).  Everything else is
 * HDD_ERR_UNSUPPORTED before the first device call, as the reference's `available = false` / NotImplemented.
 *
 * Definitions (u_h the P1 DG vector, DoF 3e + i at vertex elem_vertices[i][e]; K_T(theta) = kappa_T(theta) A_T):
 *   I_OS u_h    Oswald interpolation: at a vertex the arithmetic mean of the DG values of the elements around it (taken
 *               about the first of them in ascending element order: first + sum(u_k - first) / m), 0 at every vertex of
 *               a boundary face
 *   eta_NC,T^2  |T| g^T K_T(theta_bar) g, g = grad(u_h - I_OS u_h)
 *   eta_R,T^2   h_T^2 / (pi^2 lambda_min(K_T(theta_mu))) int_T (f - P0 f)^2: h_T the longest edge, P0 f the element mean by
 *               the simplex rule of order ord(f) + 2, the integral by the rule of order 2 ord(f) + 2; exactly 0 for a
 *               CONST / PER_ELEM / absent force
 *   F_T,e       the outward flux of the RT0 reconstruction t_h through face e with unit outer normal n,
 *                 -|e| (w- K- grad u- + w+ K+ grad u+) . n + (sigma_inner gamma / |e|^beta) int_e (u- - u+)    interior
 *                 -|e| K grad u . n + (sigma_boundary delta / |e|^beta) int_e u                                  boundary
 *               delta+- = n . K+-(theta_mu) n, w- = delta+ / (delta+ + delta-), w+ = delta- / (delta+ + delta-), gamma =
 *               delta+ delta- / (delta+ + delta-), sigma and beta from hdd_swipdg_params.  For kappa = 1 these are the
 *               weights and the penalty of the scheme itself, and sum_e F_T,e is the sum of the three rows of element T
 *               of (sum_q theta_mu,q A_q) u; for a kappa that varies the scheme takes delta from the tensor alone and
 *               multiplies its penalty by kappa- kappa+, so the two differ (F_T,e + F_T',e' = 0 holds always);
 *               t_h(x) = sum_e F_T,e / (2 |T|) (x - p_e), p_e the vertex opposite e
 *   eta_DF,T^2  int_T (grad u_h + Khat^-1 t_h)^T Khat (grad u_h + Khat^-1 t_h), Khat = K_T(theta_hat), by the three edge
 *               midpoints (exact)
 *   eta_T^2     eta_NC,T^2 + (eta_R,T + eta_DF,T)^2
 * so that eta_ESV2007 = sqrt(sums[3]) and eta_ESV2007_alt = sqrt(sums[0]) + sqrt(sums[1]) + sqrt(sums[2]). */
typedef struct hdd_estimator hdd_estimator;
/* Builds, once per mesh, the device tables of the kernels from the host view: the vertex -> (element, local vertex) CSR
 * with entries in ascending element id and the boundary-vertex flags (12 B per element, 9 B per vertex).  The only
 * place that allocates.  HDD_ERR_UNSUPPORTED (before the first device call) for a grid that is not a 2d simplex grid, a
 * view with ghosts, a Neumann face.  ctx == NULL: a host-only estimator (sizes, no device tables), which
 * hdd_estimator_workspace accepts and hdd_swipdg_estimate rejects after its other checks. */
int hdd_estimator_create(hdd_ctx* ctx, const hdd_local* l, hdd_estimator** out);
void hdd_estimator_destroy(hdd_estimator* est);
/* doubles of caller workspace hdd_swipdg_estimate needs: the Oswald value of every vertex, four partial sums per 256
 * elements and their totals; 0 for a null estimator */
int64_t hdd_estimator_workspace(const hdd_estimator* est);
/* on != 0: the calls that follow compute the reference's eta_R_ESV2007_* in place of eta_R (LocalResidualESV2007Star,
 * estimators/swipdg.hh:320-470): div t_h = sum_e F_T,e / |T| stands for P0 f, eta_R*,T^2 = h_T^2 / (pi^2 lambda_min)
 * int_T (f - div t_h)^2 by the rule of order 2 ord(f) + 2, for every force kind (an absent force is f = 0).  It takes
 * the place of eta_R,T^2 in d_local, sums[1] and eta_T^2.  Default off. */
int hdd_estimator_set_residual_star(hdd_estimator* est, int32_t on);
/* mesh: the device mesh of the estimator's view, with elem_vertices / vertex_coords (HDD_ERR_INVALID without).  kappa
 * [n_comp]; theta_mu (flux reconstruction, residual), theta_bar (nonconformity), theta_hat (diffusive flux): host
 * [n_comp]; theta_mu == NULL: all ones, as in hdd_operator_apply; theta_bar / theta_hat == NULL: theta_mu.
 * d_u: device [3 n].  d_work: device, n_work >= hdd_estimator_workspace doubles, 16-byte aligned.
 * Outputs: d_local NULL or device [4][n] (eta_NC,T^2, eta_R,T^2, eta_DF,T^2, eta_T^2); d_flux NULL or device [3][n], F_T,e
 * in the mesh's face order (the RT0 reconstruction itself: a conservative velocity field); d_oswald NULL or device
 * [n_vertices]; sums host [4], the four sums over T.  What is computed does not depend on which outputs are NULL.
 * Two launches (a lane per vertex, a lane per element) and the final reduction.  No atomics: the vertex means are a
 * gather through the CSR and the sums are two-stage in a fixed order -- element e is lane e % 256 of workgroup e / 256,
 * a workgroup adds v[t] += v[t + s] for s = 128 .. 1 (lanes without an element hold 0), then lane t of one workgroup
 * adds the partial sums t, t + 256, ... in order and the same tree follows -- so every output is bit-identical from
 * call to call.  Allocates nothing; SYNCHRONISES `stream` once to return the sums (through the pinned bytes the context
 * owns since its creation); one stream at a time per context.
 * HDD_ERR_INVALID (every argument check precedes the first device call) for a null ctx / est / mesh / kappa / tensor /
 * params / d_u / d_work / sums, n_comp outside 1..HDD_MAX_COMP, a mesh of another size than the estimator's or without
 * its vertex-indexed geometry, neighbours or face_info, a PER_ELEM function without values, n_work too small, a
 * host-only estimator; HDD_ERR_UNSUPPORTED for quadrilaterals / hexahedra, degree > 1, a view with ghosts, a smooth
 * kappa, a force whose two rules have more than 96 points together (ord(f) > 6). */
int hdd_swipdg_estimate(hdd_ctx* ctx, const hdd_estimator* est, const hdd_mesh* mesh, const hdd_scalar_fn* kappa,
                        int32_t n_comp, const double* theta_mu, const double* theta_bar, const double* theta_hat,
                        const hdd_tensor_fn* tensor, const hdd_scalar_fn* force, const hdd_swipdg_params* params,
                        const double* d_u, double* d_work, int64_t n_work, double* d_local, double* d_flux,
                        double* d_oswald, double* sums, void* stream);
/* the kernels of this thread's last hdd_swipdg_estimate or hdd_block_swipdg_estimate ("" if none), e.g.
 * "oswald_vertex_kernel + esv2007_element_kernel<beta1, cos_product>" (beta == 1 is specialised: "pow" otherwise;
 * the force: no_force, cos_product, generic_force); the block call's is
 * "oswald_vertex_kernel + esv2007_element_kernel<beta1, cos_product, block> + block_segment_kernel + block_total_kernel" */
const char* hdd_last_estimate_kernels(void);

/* ---------------------------------------------------------------------------------------------- */
/* localized estimator -- Estimators::BlockSWIPDG (estimators/block-swipdg.hh:118-328, 546-561,      */
/* 721-890): eta_NC_OS2014, eta_R_OS2014 (eta_R_OS2014_* with hdd_estimator_set_residual_star),       */
/* eta_DF_OS2014, eta_OS2014 and the per-subdomain indicators of estimate_local.  Additive to ABI 8.   */
/* ---------------------------------------------------------------------------------------------- */
/* A segment is a contiguous element range [bounds[s], bounds[s + 1]) of the estimator's whole-grid view; the view is
 * subdomain-major, so a subdomain (or several) is a segment (hdd_grid_subdomain_range).  The segments partition [0, n).
 * Five parameter roles: theta_mu, theta_bar, theta_hat as in hdd_swipdg_estimate, theta_min / theta_max the reference's
 * parameter_range_min / parameter_range_max.
 *
 * Per element T (d_local [4][n] of the block call):
 *   row 0  eta_NC,T^2 and row 2 eta_DF,T^2: those of hdd_swipdg_estimate, bit for bit (LocalNonconformityOS2014 and
 *          LocalDiffusiveFluxOS2014 are the ESV2007 classes), as are d_flux and d_oswald
 *   row 1  r_T = int_T (f - P0 f)^2 by the two simplex rules of eta_R,T^2, without its factor h_T^2 / (pi^2 lambda_min);
 *          with residual_star on, div t_h stands for P0 f (eta_R_OS2014_*)
 *   row 3  m_T = min(kappa_T(theta_min), kappa_T(theta_max)) lambda_min(A_T)
 * Per segment s (d_segments [4][S]):
 *   row 0  N_s = sum_{T in s} eta_NC,T^2          row 2  D_s = sum_{T in s} eta_DF,T^2
 *   row 1  R_s = diam_s^2 / (pi^2 min_{T in s} m_T) sum_{T in s} r_T, diam_s the largest distance between two vertices of
 *          the segment's elements
 *   row 3  the indicator of estimate_local, 3 / sqrt(alpha_bar) (sqrt(gamma_bar) N_s + R_s + gamma_tilde D_s) / eta^2 with alpha_bar =
 *          alpha(mu, mu_bar), gamma_bar = gamma(mu, mu_bar), gamma_tilde = max(sqrt(gamma(mu, mu_hat)), 1 / sqrt(alpha(mu, mu_hat)))
 *          (block-swipdg.hh:873-887, its exponents as they stand); 0 in every segment when eta = 0 (all of N_s, R_s, D_s
 *          vanish: e.g. u_h = 0 without a force), where the reference divides 0 by 0
 * Global (sums [4], host): sum_s N_s, sum_s R_s, sum_s D_s and eta^2, eta_OS2014 = 1 / sqrt(alpha_bar) (sqrt(gamma_bar) eta_NC +
 * eta_R + gamma_tilde eta_DF) with eta_NC = sqrt(sums[0]), eta_R = sqrt(sums[1]), eta_DF = sqrt(sums[2]).
 * alpha(mu, mu') = min_q theta_q(mu) / theta_q(mu'), gamma(mu, mu') = max_q of the same ratio: the definition of the
 * OS2014 paper for an affinely decomposed diffusion factor with non-negative components (the reference takes both from
 * dune-pymor).  The reference asserts that they are positive: a non-positive theta in any role is HDD_ERR_INVALID.
 *
 * Sums, in a fixed order and without atomics, bit-identical from call to call: a segment's sum is the two-stage sum of
 * hdd_swipdg_estimate applied to its slice -- chunks of 256 elements counted from the segment's first element, the tree
 * v[t] += v[t + s], s = 128 .. 1, per chunk, then lane t adds the chunk sums t, t + 256, ... in order and the same tree
 * follows -- so it does not depend on how the rest of [0, n) is cut, and with the one segment [0, n) rows 0 and 2 are
 * sums[0] and sums[2] of hdd_swipdg_estimate.  The totals: lane t adds the segments s = t, t + 256, ... in order, then the
 * tree.  Four launches whatever S: a lane per vertex, a lane per element over segment-aligned chunks, a workgroup per
 * segment over its chunk sums, one workgroup for the totals, eta^2 and the scaling of the indicators. */
/* bounds: host [n_segments + 1], strictly ascending, bounds[0] == 0, bounds[n_segments] == n (HDD_ERR_INVALID
 * otherwise, with the tables of the last valid call kept).  Builds the per-segment host and device tables (bounds,
 * chunk prefix, diameters: 24 B per segment); the diameters by the convex hull of the segment's distinct vertices,
 * O(V log V), from the host geometry every estimator keeps since its creation (12 B per element, 16 B per vertex).  Allocates, so that the block call does not.  Works on a host-only estimator (no device tables).
 * n_segments == 0 clears the tables (bounds may be NULL). */
int hdd_estimator_set_segments(hdd_estimator* est, int64_t n_segments, const int64_t* bounds);
/* out: host [n_segments], diam_s; HDD_ERR_INVALID without segments */
int hdd_estimator_segment_diameters(const hdd_estimator* est, double* out);
/* doubles of caller workspace hdd_block_swipdg_estimate needs with the segments set now: the Oswald values, four
 * partials per chunk, the totals, four values per segment; 0 for a null estimator or without segments */
int64_t hdd_estimator_blocks_workspace(const hdd_estimator* est);
/* out = alpha(mu, mu_bar), gamma(mu, mu_bar), alpha(mu, mu_hat), gamma(mu, mu_hat), max(sqrt(gamma(mu, mu_hat)),
 * 1 / sqrt(alpha(mu, mu_hat))); host [n_comp] each, theta_mu NULL: all ones, theta_bar / theta_hat NULL: theta_mu.  Pure
 * host function.  HDD_ERR_INVALID for n_comp outside 1..HDD_MAX_COMP or a non-positive component. */
int hdd_os2014_factors(int32_t n_comp, const double* theta_mu, const double* theta_bar, const double* theta_hat,
                       double out[5]);
/* The arguments, scope and checks of hdd_swipdg_estimate (every check before the first device call), and: theta_min /
 * theta_max host [n_comp], NULL: theta_mu; d_work of n_work >= hdd_estimator_blocks_workspace doubles; d_segments NULL or
 * device [4][n_segments].  The indicators are scaled on the device: the four sums alone cross to the host, behind the one
 * synchronisation of `stream`.  Additionally HDD_ERR_INVALID without segments and for a non-positive theta. */
int hdd_block_swipdg_estimate(hdd_ctx* ctx, const hdd_estimator* est, const hdd_mesh* mesh, const hdd_scalar_fn* kappa,
                              int32_t n_comp, const double* theta_mu, const double* theta_bar, const double* theta_hat,
                              const double* theta_min, const double* theta_max, const hdd_tensor_fn* tensor,
                              const hdd_scalar_fn* force, const hdd_swipdg_params* params, const double* d_u,
                              double* d_work, int64_t n_work, double* d_local, double* d_flux, double* d_oswald,
                              double* d_segments, double* sums, void* stream);

/* ---------------------------------------------------------------------------------------------- */
/* sharded BlockSWIPDG (SURVEY.md 8(b) hdd_block_assemble_sharded, 8(e)): one process (or thread) per  */
/* GPU owns a contiguous range of subdomains and assembles their rows -- A_ss and A_ss,nn are written  */
/* by the owner of ss (block-swipdg.hh:355-382, coupling 1270-1326, boundary 1136-1179), so there is  */
/* no reduction; the only exchange is the face halo (per-element records of the ghost elements).      */
/* ---------------------------------------------------------------------------------------------- */
typedef struct hdd_comm hdd_comm;
typedef struct hdd_shard hdd_shard;

#define HDD_RCCL_ID_BYTES 128   /* sizeof(ncclUniqueId) */

/* Host transport: moves n_peers messages (host memory, doubles) and returns HDD_OK; message k goes to
 * rank peers[k] (send[k], send_count[k] doubles) and the message of that rank lands in recv[k]
 * (recv_count[k] doubles).  Called synchronously from hdd_comm_post on the caller's thread (e.g. MPI,
 * gloo or an in-process mailbox). */
typedef int (*hdd_host_exchange_fn)(void* user, int32_t n_peers, const int32_t* peers, const double* const* send,
                                    const int64_t* send_count, double* const* recv, const int64_t* recv_count);

/* RCCL (librccl, resolved at run time in the calling process: PyTorch-ROCm's copy when it is loaded)
 * -- ncclGetUniqueId on one rank, broadcast the HDD_RCCL_ID_BYTES bytes, ncclCommInitRank on every rank */
int hdd_rccl_get_unique_id(void* id);
int hdd_comm_create_rccl(const void* id, int32_t nranks, int32_t rank, int32_t hip_device, hdd_comm** out);
/* wrap an existing ncclComm_t (not destroyed by hdd_comm_destroy) */
int hdd_comm_wrap_rccl(void* nccl_comm, int32_t hip_device, hdd_comm** out);
/* host-staged transport: device -> pinned host -> fn -> device (synchronous; rehearsal / tests / MPI) */
int hdd_comm_create_host(hdd_host_exchange_fn fn, void* user, int32_t hip_device, hdd_comm** out);
/* In-process device transport (ABI 7): nranks ranks of ONE process, one thread each (any devices, one device
 * allowed), exchanging device buffers with RCCL's stream schedule -- the exchange runs on the communicator's
 * transfer stream: it waits for each source's packed event, copies its messages (hipMemcpyAsync) into the
 * receive buffers, records a "copied" event, and completes (the event hdd_comm_wait joins) once every
 * destination has copied this rank's sends; so the sharded step takes exactly the branch it takes over RCCL.
 * hdd_comm_post blocks the calling thread until every source rank has posted (a host rendezvous; 120 s
 * timeout, then every waiting rank returns HDD_ERR_INVALID).  The hub is reference counted: destroying it
 * while communicators still use it is allowed. */
typedef struct hdd_device_hub hdd_device_hub;
int hdd_device_hub_create(int32_t nranks, hdd_device_hub** out);
void hdd_device_hub_destroy(hdd_device_hub* hub);
int hdd_comm_create_device(hdd_device_hub* hub, int32_t rank, int32_t hip_device, hdd_comm** out);
void hdd_comm_destroy(hdd_comm* comm);
/* Post one exchange of device buffers: it starts after the work enqueued on `stream` so far; RCCL runs
 * it on the communicator's own transfer stream (ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd), so
 * work enqueued on `stream` afterwards overlaps it until hdd_comm_wait(comm, stream). */
int hdd_comm_post(hdd_comm* comm, int32_t n_peers, const int32_t* peers, const double* const* d_send,
                  const int64_t* send_count, double* const* d_recv, const int64_t* recv_count, void* stream);
/* The same exchange ordered on `stream` itself: RCCL runs the group send/recv on `stream` (no transfer stream, no
 * cross-stream events -- for callers that overlap nothing with it, as the serial sharded step); other transports
 * behave as hdd_comm_post.  hdd_comm_wait(comm, stream) is then a no-op on that stream. */
int hdd_comm_post_direct(hdd_comm* comm, int32_t n_peers, const int32_t* peers, const double* const* d_send,
                         const int64_t* send_count, double* const* d_recv, const int64_t* recv_count, void* stream);
/* make `stream` wait for the receives of the last hdd_comm_post (no host blocking with RCCL) */
int hdd_comm_wait(hdd_comm* comm, void* stream);

typedef struct {
  int64_t n_local, own_begin, own_end, n_ghost, global_first;   /* as hdd_local_info */
  int64_t n_rows, n_cols, nnz;      /* owned rows (nb per owned element), global columns, pattern nnz */
  int32_t rank, nranks, s_begin, s_end, n_peers, nb;
  int64_t n_tiles, n_tiles_interior, n_tiles_boundary;   /* 64-element tiles of the owned elements */
  int64_t halo_send, halo_recv;     /* elements sent / ghost elements received per exchange */
  int64_t halo_faces;               /* faces between an owned and a ghost element */
  int64_t halo_elements;            /* owned elements with a ghost face neighbour (the fixup pass) */
} hdd_shard_info;

/* Rank `rank` of `nranks` owns the subdomains s with owner[s] == rank, which must form one contiguous
 * range (owner == NULL: contiguous near-equal ranges, [n_sub r / nranks, n_sub (r+1) / nranks)).  Builds
 * the rank-local mesh (host work O(owned + ghost elements): the structured grids are implicit, nothing
 * global is materialised), uploads it with the ghost geometry, the halo plan, the device send lists and
 * the interior / halo-boundary 64-element tile lists. */
int hdd_shard_create(hdd_ctx* ctx, const hdd_grid* g, int32_t nranks, int32_t rank, const int32_t* owner,
                     hdd_shard** out);
/* ctx == NULL: a host-only shard (local mesh, halo plan, tile lists; no device arrays) -- what a rank can
 * inspect without a GPU, e.g. to check the halo protocol on CPU ranks (tests/test_distributed.py) */
void hdd_shard_destroy(hdd_shard* sh);
int hdd_shard_get_info(const hdd_shard* sh, hdd_shard_info* out);
/* the halo plan (host copies): peers [n_peers] ascending; send lists = local element indices, peer k's
 * part at [send_prefix[k], send_prefix[k+1]) of send_idx [halo_send] (send_prefix [n_peers+1]); the
 * message from peer k fills ghost columns recv_col0[k] .. recv_col0[k] + (recv_prefix[k+1] - recv_prefix[k])
 * (recv_prefix [n_peers+1], recv_col0 [n_peers]).  Any pointer may be NULL. */
int hdd_shard_halo_lists(const hdd_shard* sh, int32_t* peers, int64_t* send_prefix, int32_t* send_idx,
                         int64_t* recv_prefix, int64_t* recv_col0);
/* the 64-element tiles (relative to own_begin) without / with a ghost face neighbour:
 * interior [n_tiles_interior], boundary [n_tiles_boundary]; either may be NULL */
int hdd_shard_tile_lists(const hdd_shard* sh, int32_t* interior, int32_t* boundary);
/* the shard's device mesh (shard-owned arrays; usable with every hdd_* device call) */
int hdd_shard_mesh(const hdd_shard* sh, hdd_mesh* out);
/* host arrays [n_local]: global element ids; element barycentres [dim][n_local] (coefficient lookup) */
int hdd_shard_global_ids(const hdd_shard* sh, int64_t* global_id);
int hdd_shard_centers(const hdd_shard* sh, double* centers);
/* device pattern of the owned rows (global columns) into caller buffers d_row_ptr [n_rows+1],
 * d_col [nnz], d_elem_ptr [own_end-own_begin+1]; synchronises `stream` */
int hdd_shard_pattern_fill(hdd_ctx* ctx, const hdd_shard* sh, int64_t* d_row_ptr, int32_t* d_col,
                           int64_t* d_elem_ptr, void* stream);

enum {
  HDD_SHARD_NO_OVERLAP = 1,     /* exchange, then assemble every tile (the default on Q1 shards; P1 shards overlap
                                   the assembly with the halo) */
  HDD_SHARD_HALO_GEOMETRY = 2,  /* also send the ghost vertex coordinates (default: geometry is rank-local) */
  HDD_SHARD_NO_HALO = 4,        /* ghost columns already valid (static coefficients): no exchange at all */
  HDD_SHARD_NO_TRANSFER = 8,    /* timing studies only: pack and split tile launches as in an exchange, one
                                   loopback kernel instead of the transfer -- the unpack, reading the send buffer
                                   (a copy per peer first when send and receive counts differ) (comm may be NULL; the
                                   ghost columns receive the rank's own send buffers, i.e. wrong values) -- an
                                   upper bound of the GPU-side cost of the sharded step */
  HDD_SHARD_SPLIT_TILES = 16,   /* overlap by tiles: interior tiles during the exchange, the tiles with a
                                   ghost-adjacent element after it -- the default for P1 shards with two peers;
                                   other P1 shards default to every tile during the exchange and the ghost-adjacent
                                   ELEMENTS again, off-stream, in place (HDD_SHARD_FIX_INPLACE); Q1 shards to the
                                   serial step (HDD_SHARD_NO_OVERLAP; measured fastest) */
  HDD_SHARD_FIX_INLINE = 32,    /* study (round 3 A/B): the ghost-adjacent elements recomputed on `stream` after
                                   the wait (default: on the transfer stream right after the receives, beside the
                                   assembly) */
  HDD_SHARD_FIX_SCATTER = 64,   /* the off-stream fixup into a side buffer, copied into place by one kernel after the
                                   join (the assembly's tiles store every row block; Q1: a value-major buffer, one
                                   full-range half-image launch beside the element pass) */
  HDD_SHARD_FIX_INPLACE = 128,  /* the off-stream fixup in place, the assembly's tiles skip those row blocks (a SKIP
                                   launch; Q1: the pack on `stream` ahead of it): the default on P1 end ranks */
  HDD_SHARD_LAUNCH_LAST = 256   /* ablation builds only (round 3's order, measured and rejected): with the in-place
                                   fixup, enqueue the full-range launch after the halo work instead of before it;
                                   the product library ignores it */
};
/* One sharded assembly step -- the LHS of BlockSWIPDG::init() for the owned subdomains: pack the halo
 * records (per-element tensor / kappa rows, [+ coordinates]) of the elements the peers need -> post the
 * exchange, one message per (peer, halo row), received straight into the ghost columns (the ghosts of one
 * owner are contiguous, recv_col0) -> every tile except the row blocks that read a ghost column; those
 * elements (hdd_shard_info.halo_elements of them, one lane each) are computed on
 * the transfer stream as soon as their halo has landed, concurrently with the assembly, whose tiles leave those
 * row blocks to them -> join.  The per-element arrays
 * of `kappa` / `tensor` must span n_local columns: their owned columns are read and their GHOST COLUMNS ARE
 * WRITTEN by the receives.  comm may be NULL when the shard has no peers. */
int hdd_block_assemble_sharded(hdd_ctx* ctx, hdd_shard* sh, hdd_comm* comm, const hdd_scalar_fn* kappa,
                               int32_t n_comp, const hdd_tensor_fn* tensor, const hdd_swipdg_params* params,
                               const hdd_csr* pattern, double* const* d_vals, uint32_t flags, void* stream);

/* Watchdog of the sharded step (ABI 8).  A lost or stalled peer shows as a step that never completes on the device
 * (RCCL waits inside its kernels), so instead of blocking in a device synchronize a rank can poll the events of its
 * last step with a deadline and report where it stopped.  Stages in pipeline order: */
enum {
  HDD_STAGE_COMPLETE = 0,
  HDD_STAGE_PACK = 1,       /* the halo pack kernel (the event the transfer starts from) */
  HDD_STAGE_EXCHANGE = 2,   /* the group send / recv with the halo peers */
  HDD_STAGE_ELEMENTS = 3,   /* the ghost-adjacent element pass behind the receives */
  HDD_STAGE_ASSEMBLY = 4    /* the tile launch(es) and the join on `stream` (up to the last hdd_block_step_mark) */
};
/* record the marker event on `stream` (after the steps to watch) */
int hdd_block_step_mark(hdd_shard* sh, void* stream);
/* non-blocking: *stage = the first stage of the last step (and the marker) whose event has not completed */
int hdd_block_step_query(hdd_shard* sh, int32_t* stage);
const char* hdd_block_stage_name(int32_t stage);
/* mark, then poll until every stage has completed or timeout_s has passed: HDD_ERR_TIMEOUT with a message naming
 * the rank, the stage and the halo peers (hdd_last_error) */
int hdd_block_step_sync(hdd_shard* sh, void* stream, double timeout_s);
/* Error injection (tests of the watchdog): the next hdd_comm_post of `rank` on this hub publishes sends that complete
 * only when hdd_device_hub_release() opens a device-side gate, or after max_seconds (a one-wave kernel polling a
 * host word; it always ends) -- a peer whose sends do not arrive. */
int hdd_device_hub_stall(hdd_device_hub* hub, int32_t rank, double max_seconds);
int hdd_device_hub_release(hdd_device_hub* hub);

#ifdef __cplusplus
}
#endif
#endif /* HDD_H */
