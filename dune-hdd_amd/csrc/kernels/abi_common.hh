// dune-hdd_amd/csrc/kernels/abi_common.hh -- what the ABI entry points share (internal): one validator per fact
// and the fillers of the kernel argument blocks.  Every validator takes the entry point's name (`who`), sets the
// per-thread message and returns the status; the entry points call them in their own (documented) order.
#pragma once
#include <algorithm>
#include <string>

#include "ctx.hh"
#include "swipdg_kernels.hh"

#pragma GCC visibility push(hidden)   // internal: none of this is an exported symbol
namespace hdd {
namespace abi {

inline int fail(int code, const char* who, const char* what) { return set_error(code, std::string(who) + ": " + what); }

inline int fn_order(const hdd_scalar_fn& f)
{
  return (f.kind == HDD_FN_SINUSOID || f.kind == HDD_FN_COS_PRODUCT || f.kind == HDD_FN_FLATTOP) ? f.order : 0;
}

// basis functions per element; faces per element (0: unknown element type)
inline int mesh_nb(int32_t elem_type, int degree)
{
  return elem_type == HDD_SIMPLEX ? 3 : (elem_type == HDD_CUBE ? 4 : (degree + 1) * (degree + 1) * (degree + 1));
}
inline int mesh_faces(int32_t elem_type)
{
  return elem_type == HDD_SIMPLEX ? 3 : (elem_type == HDD_CUBE ? 4 : (elem_type == HDD_HEX ? 6 : 0));
}

inline int check_elem_type(const char* who, const hdd_mesh* m)
{
  return mesh_faces(m->elem_type) ? HDD_OK : fail(HDD_ERR_UNSUPPORTED, who, "unknown element type");
}

inline int check_own_range(const char* who, const hdd_mesh* m)
{
  if (m->own_begin < 0 || m->own_end > m->n_local || m->own_begin > m->own_end)
    return fail(HDD_ERR_RANGE, who, "0 <= own_begin <= own_end <= n_local violated");
  return HDD_OK;
}

// 2d meshes carry P1 / Q1, HDD_HEX p = 1..3 (a degree below 1 counts as 1); *deg: the degree in use
inline int check_degree(const char* who, const hdd_mesh* m, int* deg)
{
  *deg = m->elem_type == HDD_HEX ? std::max(1, int(m->degree)) : 1;
  if (m->elem_type != HDD_HEX && m->degree > 1)
    return fail(HDD_ERR_UNSUPPORTED, who, "2d meshes carry P1 / Q1 only (degree <= 1)");
  if (*deg > 3) return fail(HDD_ERR_UNSUPPORTED, who, "HDD_HEX supports p = 1..3");
  return HDD_OK;
}

inline int check_pattern_rows(const char* who, const hdd_csr* pattern, int nb, const hdd_mesh* m)
{
  if (pattern->n_rows != int64_t(nb) * (m->own_end - m->own_begin))
    return fail(HDD_ERR_INVALID, who, "pattern rows != nb * owned elements");
  return HDD_OK;
}

// The reference requires a non-parametric, non-empty tensor (swipdg.hh:173-176); here the tensor is a plain
// function, so only its kind is checked.
inline int check_tensor_kind(const char* who, const hdd_tensor_fn* t)
{
  if (t->kind != HDD_TENSOR_CONST && t->kind != HDD_TENSOR_ISO_PER_ELEM && t->kind != HDD_TENSOR_SYM_PER_ELEM)
    return fail(HDD_ERR_UNSUPPORTED, who, "unknown tensor kind");
  return HDD_OK;
}

inline int check_tensor(const char* who, const hdd_tensor_fn* t)   // t may be null (no tensor)
{
  if (t && t->kind != HDD_TENSOR_CONST && !t->per_elem) return fail(HDD_ERR_INVALID, who, "tensor per_elem missing");
  return HDD_OK;
}

inline int check_fn_per_elem(const char* who, const hdd_scalar_fn* f)   // f may be null (no function)
{
  if (f && f->kind == HDD_FN_PER_ELEM && !f->per_elem)
    return fail(HDD_ERR_INVALID, who, "per_elem function without values");
  return HDD_OK;
}

// HDD_FN_FLATTOP needs its box table and a 2d mesh.  The entry points have always reported these two failures with
// different status codes, so the codes are arguments; f may be null.
inline int check_flattop(const char* who, const hdd_scalar_fn* f, int32_t elem_type, int table_code, int hex_code)
{
  if (!f || f->kind != HDD_FN_FLATTOP) return HDD_OK;
  if (f->n_table < 0 || (f->n_table > 0 && !f->table)) return fail(table_code, who, "FLATTOP box table missing");
  if (elem_type == HDD_HEX) return fail(hex_code, who, "FLATTOP needs a 2d mesh");
  return HDD_OK;
}

inline int check_vertex_arrays(const char* who, const hdd_mesh* m)
{
  if (!m->elem_vertices != !m->vertex_coords)
    return fail(HDD_ERR_INVALID, who, "mesh elem_vertices / vertex_coords: both or neither");
  return HDD_OK;
}

// Whether a call reads the 2d mesh's vertex-indexed geometry (elem_vertices / vertex_coords) instead of the
// element-major coords; HDD_VARIANT_ELEMENT_MAJOR keeps the element-major coords (cross-check).  The callers differ:
//   assembly: any 2d mesh, offsets32 -- the tile kernels read it with 32-bit byte offsets, so larger meshes
//             (vx_offsets_fit) take the element-major coords;
//   products: simplex_only (the tile driver's product kernels have a vertex-indexed form for P1 alone), offsets32;
//   RHS:      any 2d mesh, no size limit -- rhs.hip indexes vertex_coords through 64-bit pointers.
inline bool use_vertex_geometry(const hdd_ctx* ctx, const hdd_mesh* m, bool simplex_only, bool offsets32)
{
  if (!m->elem_vertices || m->elem_type == HDD_HEX || (ctx->variant & HDD_VARIANT_ELEMENT_MAJOR)) return false;
  if (simplex_only && m->elem_type != HDD_SIMPLEX) return false;
  return !offsets32 || vx_offsets_fit(m->n_local);
}

// the mesh, pattern and context fields of the tile driver's arguments (everything but coefficients, lists, outputs)
inline dev::AssembleArgs mesh_args(const hdd_ctx* ctx, const hdd_mesh* m, const hdd_csr* pattern)
{
  dev::AssembleArgs a{};
  a.elem_type = m->elem_type;
  a.n_local = m->n_local;
  a.own_begin = m->own_begin;
  a.own_end = m->own_end;
  a.coords = m->coords;
  a.nbrs = m->neighbors;
  a.finfo = m->face_info;
  a.elem_ptr = pattern->elem_ptr;
  a.n_cu = ctx->n_cu;
  a.debug_flags = ctx->debug_flags;   // profiling ablations only
  a.variant = ctx->variant;
  a.wgcu = ctx->wgcu;
  return a;
}

// tensor (null: HDD_TENSOR_CONST zero), penalty parameters
inline void set_coefficients(dev::AssembleArgs& a, const hdd_tensor_fn* tensor, const hdd_swipdg_params* p)
{
  a.tkind = tensor ? tensor->kind : HDD_TENSOR_CONST;
  a.tc0 = tensor ? tensor->c[0] : 0.0;
  a.tc1 = tensor ? tensor->c[1] : 0.0;
  a.tc2 = tensor ? tensor->c[2] : 0.0;
  a.tper = tensor ? tensor->per_elem : nullptr;
  a.sigma_inner = p->sigma_inner;
  a.sigma_boundary = p->sigma_boundary;
  a.beta = p->beta;
}

}  // namespace abi
}  // namespace hdd
#pragma GCC visibility pop
