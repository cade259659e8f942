// dune-hdd_amd/csrc/kernels/swipdg_device.hh -- design overview of the SWIPDG assembly kernels (comments only; no
// translation unit includes this file).  The swipdg_*.hip translation units (one per kernel family, so the
// template instantiations compile in parallel) include the parts they use:
//   swipdg_elements.hh        reference elements, rules, coefficient access, geometry, 32-bit offset loaders
//   swipdg_policy.hh          the optional capabilities of a policy (PolicyDefaults), RotImg
//   swipdg_policy_p1.hh       P1PwcPolicy, P1SmoothPolicy, P1SmoothFusedPolicy
//   swipdg_policy_generic.hh  GenericPolicy, Q1PwcPolicy, VolProductPolicy
//   swipdg_persistent.hh      the persistent tile driver and its stages, the element-list kernels
//   swipdg_launch.hh          launch_persistent and the kind dispatch helpers
//   swipdg_wave_per_row.hh    the wave-per-row fallback kernel (swipdg_assemble.hip only)
//
// CDNA4 (gfx950) kernels of the SWIPDG stiffness assembly -- the MI355X replacement of dune-gdt's
// SystemAssembler::walk() over Operators::EllipticSWIPDG (reference call sites:
// dune/hdd/linearelliptic/discretizations/swipdg.hh:218-249, 485; block-swipdg.hh:1136-1179, 1270-1326).
//
// Design:
//   * owner-computes: the rows of an element are written by the lanes that own the element; every face
//     term is evaluated by the row owner on its side (entity/entity + entity/neighbour blocks), so each
//     CSR value is written exactly once, with no atomics and no zero-fill, in one pass over the mesh;
//   * a workgroup = one tile of 64 consecutive owned elements; WPE waves per tile, wave w owns the local
//     test functions (rows) [w*RPT, (w+1)*RPT) of the 64 elements, lane = element (coalesced SoA loads);
//   * the row block of an element is contiguous in the CSR value array (sorted blocks, element-blocked
//     DoFs), so each wave stages one row of its 64 elements in LDS and streams it out with consecutive
//     lanes on consecutive values (6-12 cache lines per store instruction instead of 64);
//   * reference-element basis/quadrature tables are compile-time constants (immediates), not LDS: at
//     p = 1 they are a handful of numbers per rule;
//   * the neighbour geometry is rebuilt from the shared face vertices plus the neighbour's non-face
//     vertices (twin face / orientation from face_info), so a face gathers 2 (triangle) or 4 (quad)
//     coordinates, the neighbour's tensor and coefficient;
//   * XCD-aware tile order: consecutive tiles run on one XCD so the neighbour rows above/below a tile
//     hit that XCD's L2.
