/*
 * hermnet_hip.h -- C ABI of the MI355X (gfx950) hot-path library `libhermnet_hip.so`.
 *
 * The reference has no FFI: its hot path is reached through Python operators.
 * Each entry point below names the reference operator (file:line under
 * /root/reference) it replaces; INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add at that call site.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in `_host`;
 *   - all buffers are allocated and owned by the caller (PyTorch in our host
 *     code); the library never allocates, frees or retains them;
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work
 *     on it (no host synchronisation, graph-capturable);
 *   - return value 0 = ok, non-zero = HN_ERR_* (host code raises RuntimeError);
 *   - float = IEEE fp32 (the reference is fp32-only), indices = int32 (int64 where a parameter says so:
 *     the caller's edge_index / atomic_number / halo index lists arrive as torch LongTensors).
 *
 * ABI version 13 (`HN_ABI_VERSION` below, returned by `hermnet_abi_version`): hermnet_edge_geometry_bwd_virial, then hermnet_graph_virial / _workspace and
 * hermnet_neighbor_count_devcell, then hermnet_node_update_fwd_last / _bwd_last and hermnet_message_scatter_bwd_gedge (the
 * forms without dead work at the two ends of the layer stack), then hermnet_neighbor_batch_workspace / _count / _fill /
 * _fill_padded (the search of a batch of structures), then the host probe hermnet_host_neighbor_geometry, then hermnet_md_advance / _finish / _noise with their hermnet_host_md_* twins (the device-resident integrator), then hermnet_relax_advance / _finish with their hermnet_host_relax_* twins (the device-resident FIRE relaxation), then hermnet_md_finish_npt with its hermnet_host_md_finish_npt twin (the barostat of the device-resident integrator), then hermnet_species_expand (layer 0's node projection from a per-species table), then hermnet_neb_finish with its hermnet_host_neb_finish twin (the device-resident nudged elastic band), then hermnet_remd_finish with its hermnet_host_remd_finish twin (replica exchange), then hermnet_pimd_advance / _finish with their hermnet_host_pimd_* twins (ring-polymer path-integral MD), then hermnet_observe_frames / _msd / _rdf with their hermnet_host_observe_* twins (MD observers behind a driver's finish), then hermnet_swapmc_advance / _finish with their hermnet_host_swapmc_* twins (species-swap Monte Carlo between MD steps) were added within v13 (new entry points only, nothing
 * existing changed, so the version stays 13); v13 is ADDITIVE over v12 (hermnet_band_product / _grad_a / _grad_b / _grads, hermnet_basis_window,
 * hermnet_edge_unit, hermnet_col_sum: the training path's rbf_proj on the bucketed basis and its neighbours); v12 is ADDITIVE over v11 (hermnet_halo_proj_rows / _accumulate, ranged launches of
 * hermnet_message_scatter_bwd without the finishing launch, hermnet_set_option / _get_option in place of the library's environment
 * variables, hermnet_weight_fragments; no signature, struct or fragment format of v11 changed).  STABLE from v11 on: hn_graph,
 * hn_rbf_desc, hn_pending_grads, the frag(W) / frag16(W) weight streams, and every entry point's argument list -- later versions
 * only add entry points; v11 changes the weight fragment formats of the node chain kernels (three bf16 planes:
 * see "chain kernels on the matrix pipe"); v10 adds hermnet_shard_step_flags; v9 added the fused layer-boundary node kernels (hermnet_node_update_pre_fwd, the `gxh`
 * form of hn_pending_grads, hermnet_node_pre_fwd16 / _bwd16) and hermnet_param_guard; v8 the gradients handed down as partial sums
 * (hn_pending_grads); v7 adds the row windows of the message kernels (interior / boundary launches
 * around the halo exchange), node chain kernels for every width that is a multiple of 64 up to 512, hermnet_stream_copy, and drops
 * the float-atomic mode 3 of hermnet_halo_rows; v6 added the target mask of the neighbour search (lists of an atom shard) and the
 * row windows of the node pre kernels (halo exchange overlap); v5 replaces the stand-alone node GEMM by the node chain kernels
 * (hermnet_node_pre_fwd/_bwd, hermnet_node_update_fwd/_bwd); v4 puts the radial table in CSC order (hermnet_edge_radial_table takes the
 * graph); v3 added the deterministic halo accumulate, separate source / target row
 * spaces (HTNet) and the fused node-chain kernels; v2 added the bias-on-load arguments, LayerNorm, the energy head, the
 * CSC position gradient and the halo packing; the Python side refuses a library of another version.
 *
 * Node order.  All node-level arrays are in "relation order": atoms sorted by
 * (relation index of their element, original id); atoms whose element is not in
 * the model's element list come last.  `type_rowptr[T+1]` delimits the row range
 * of each relation; rows >= type_rowptr[T] are unknown-type atoms (sources only).
 *
 * Edge orders.  CSR: edges sorted by (row(target), original edge id).
 *               CSC: edges sorted by (relation(target), row(source), CSR position).
 */
#ifndef HERMNET_HIP_H
#define HERMNET_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HN_OK 0
#define HN_ERR_BAD_ARG 1      /* unsupported shape / null pointer */
#define HN_ERR_LDS 2          /* weight tile does not fit the 160 KiB LDS */
#define HN_ERR_LAUNCH 3       /* hipLaunchKernel / hipGetLastError failed */

#define HN_ENV_POLYNOMIAL 0   /* rmnet.py:175-193 */
#define HN_ENV_EXPONENTIAL 1  /* rmnet.py:196-208 */

/* Library / build identification (also used as the "is the native path loaded" probe).  HN_ABI_VERSION is what
 * hermnet_abi_version() of a library built from this header returns; a binder compares the two. */
#define HN_ABI_VERSION 13
int hermnet_abi_version(void);
const char* hermnet_build_info(void);

/* Options (ABI v12): process-wide integers the launchers read at every call -- tuning knobs and the alternative kernel forms
 * that tests and A/Bs compare against.  (They replace the HERMNET_* environment variables that the library read once per process
 * up to ABI v11.)  Defaults are the measured choices; a binder never needs to touch them.  Ids 0-3 (the message kernels'
 * template variants) are retired: set and get refuse them with HN_ERR_BAD_ARG. */
#define HN_OPT_FWD_ROWS 4           /* target rows per workgroup; 0 = sized by the launcher */
#define HN_OPT_BWD_ROWS 5
#define HN_OPT_BWD_CL_ROWS 6        /* channel-per-lane backward: source rows per workgroup; 0 = whole rounds of one per CU */
#define HN_OPT_BWD_LANES16 7        /* 1: the 16-lanes-per-edge backward even where the channel-per-lane form could run */
#define HN_OPT_NODE_CHAIN_WIDE 8    /* 1: widths 128 / 256 on the panelled chain kernels too */
#define HN_OPT_UPDATE_TILE16 9      /* 16-row update tiles: 0 never, 1 always, 2 (default) where they shorten the launch */
#define HN_OPT_UPDATE_TILE64_MAX 10 /* largest grid (in 64-row tiles) that takes the 64-row update kernels at width 128 */
#define HN_NUM_OPTIONS 11
int hermnet_set_option(int option, int value);
int hermnet_get_option(int option, int* value);

/* The chain kernels' weight stream from a row-major fp32 weight W [out_features][in_features], computed on the HOST (both
 * pointers are host pointers): tile_rows = 32 gives frag(W), 16 gives frag16(W) (see "chain kernels on the matrix pipe"),
 * out_features * in_features * 3 bf16 values.  The format is STABLE from ABI v11 on; this routine exists so that no binder has
 * to re-implement it (hermnet_amd/nodeops.py: weight_fragments is the same map in torch ops, checked bit for bit). */
int hermnet_weight_fragments(const float* w_host, int out_features, int in_features, int tile_rows, unsigned short* frag_host);

/* Radial-basis description shared by the message kernels:
 *   u = d * inv_rc; env(u) per rmnet.py:175-208; Gaussian taps exp(coeff*(u-offset[k])^2)
 *   (PyG GaussianSmearing as used at rmnet.py:156-158: offset = linspace(0,1,R),
 *   coeff = -0.5/(offset[1]-offset[0])^2). */
typedef struct hn_rbf_desc {
  const float* offset;   /* [R] device */
  int   num_rbf;         /* R */
  float inv_rc;          /* 1/rc */
  float coeff;           /* Gaussian coefficient (negative) */
  int   env_kind;        /* HN_ENV_* */
  int   env_p;           /* polynomial exponent p */
} hn_rbf_desc;

/* Graph in relation order (built once per neighbour list by the host code). */
typedef struct hn_graph {
  int num_nodes;              /* N */
  int num_edges;              /* E */
  int num_rel;                /* T */
  const int* type_rowptr;     /* [T+1] */
  const int* csr_rowptr;      /* [N+1]  by target row */
  const int* csr_src;         /* [E]    source row of each CSR edge */
  const int* csc_rowptr;      /* [T*N+1] by (relation(target), source row) */
  const int* csc_tgt;         /* [E]    target row of each CSC edge */
  const int* csc_pos;         /* [E]    CSR position of each CSC edge */
  /* Separate source-row space (HTNet: a target atom appears once per triadic relation, "virtual" target rows,
   * while sources stay one row per atom).  num_src = 0 and res_row = NULL: sources and targets share rows (HVNet). */
  int num_src;                /* rows of xh / vec / gxh / gvec and of csr_src, csc_rowptr ([T*num_src+1]); 0 = num_nodes */
  const int* res_row;         /* [N] source row whose (x, vec) enter the residual of target row r (rmnet.py:24-26), or NULL = r */
} hn_graph;

/* ---- A16 / K18-K19: neighbor_search (data.py:14-24; ase primitive_neighbor_list / torch_cluster
 * radius_graph on the host in the reference).  Device-side cell list, float64 arithmetic on the
 * float32 coordinates; pair (i, j, S) iff |pos_j - pos_i + S cell| < rc (strict), no (i,i,0),
 * output sorted by (i, j, Sx, Sy, Sz).  Two calls around one host read:
 *   hermnet_neighbor_count  -> total_device[0] = E, total_device[1] = flags (bit 0: an |S| component exceeded 8 --
 *                              coordinates many cells away from the cell: wrap them or use the host path; bit 1: an
 *                              atom has more pairs than the per-atom key stash holds; bit 3: the device-cell form met
 *                              a degenerate cell, see below); keeps its state in `workspace`
 *   hermnet_neighbor_fill   -> edge_index [2,E] int64, edge_shift [E,3] = shift_sign * S.  stash_ok = 1 (flag bit 1
 *                              clear): the keys stashed by the counting pass are rank-sorted per atom and decoded --
 *                              no second pass over the candidates, no global sort; stash_ok = 0: two-pass form through
 *                              `keys` [E] (may be NULL when stash_ok = 1).
 * cell_host: 9 doubles (rows = lattice vectors) on the HOST, or NULL for an open system, in which
 * case lo_host/hi_host give the bounding box of the coordinates.  source_first = 1 writes rows
 * [j; i] (radius_graph convention: source, target), 0 writes [i; j] (the reference's periodic path).
 * target_ok (ABI v6; NULL = every atom): [num_atoms] bytes, only pairs whose TARGET atom (row 1 of edge_index) is
 * flagged are counted and listed -- the list of an atom shard (owned + halo atoms in, edges into owned atoms out);
 * pass the same pointer to both calls. */
/* hermnet_neighbor_fill_padded (ABI v7; SURVEY 8(f) row 1: no host round-trip inside an MD step): instead of reading E
 * between the two calls, the caller provides `capacity` columns; the pairs found fill the first E of them, the rest
 * become NULL edges (-1, -1; shift 0), and total_device = (E, flags) is written for a read at the END of the step
 * (flags as above, plus bit 2: E > capacity).  With bit 1 or 2 set the list is incomplete: repeat the search in its
 * two-call form with a larger capacity.  With bit 0 set it is incomplete too: E counts every pair, and a pair whose
 * shift has a component beyond +-8 takes a NULL edge at the end of its atom's columns -- every other column is a pair
 * with the shift it has; the host list answers such coordinates.
 * hermnet_build_relations files NULL edges behind every row (they are in no CSR /
 * CSC segment), so every kernel of the step runs on the padded arrays with num_edges = capacity -- a fixed launch
 * geometry: search + step can be captured into ONE hipGraph that stays valid across list rebuilds.  Call after
 * hermnet_neighbor_count on the same workspace. */
int hermnet_neighbor_fill_padded(int num_atoms, void* workspace, size_t workspace_bytes, long capacity, float shift_sign,
                                 int source_first, long* edge_index /* [2, capacity] */, float* edge_shift /* [capacity, 3] */,
                                 long* total_device /* [2] */, void* stream);
size_t hermnet_neighbor_workspace(int num_atoms);      /* with the largest stash slot (160 keys per atom: 1.3 kB/atom) */
/* ... or with a smaller one (8 .. 160 keys per atom): every call of a search derives the slot size from the workspace
 * size it is handed, so the workspace a caller allocates decides it.  An atom with more pairs than the slot holds sets
 * flag bit 1: the exact search then takes its two-pass form, the padded one must be repeated with a larger slot. */
size_t hermnet_neighbor_workspace_for(int num_atoms, int stash_per_atom);
int hermnet_neighbor_count(const float* pos, int num_atoms, const double* cell_host, const double* lo_host,
                           const double* hi_host, double rc, void* workspace, size_t workspace_bytes,
                           const unsigned char* target_ok, long* total_device /* [2] */, void* stream);
/* The counting pass of a periodic cell that lives in DEVICE memory (ABI 13, additive): `cell` [9] float32, rows = lattice
 * vectors.  A single-thread kernel builds the search geometry (inverse, plane spacings, bin grid, reach, coarsening) from it
 * in float64 exactly as the host does for hermnet_neighbor_count, so for the same float32 cell values the list is bit for
 * bit the same; nothing about the cell is baked into the launches (those that follow the bin count are sized by the bound
 * the workspace is carved for), so search + step captured into one hipGraph follow a cell that changes between replays.
 * Follow it with hermnet_neighbor_fill_padded on the same workspace.  A cell the host form refuses with HN_ERR_BAD_ARG
 * (singular, or so small that the cutoff reaches beyond 8 bins) raises flag bit 3 (value 8) in total_device[1] instead:
 * the kernels then run on an inert geometry (no pair is listed, nothing is read or written out of bounds) and the caller
 * must discard the step.  HN_ERR_BAD_ARG: num_atoms <= 0, rc <= 0, a missing pointer, a workspace too small. */
int hermnet_neighbor_count_devcell(const float* pos, int num_atoms, const float* cell, double rc, void* workspace,
                                   size_t workspace_bytes, const unsigned char* target_ok, long* total_device /* [2] */,
                                   void* stream);
int hermnet_neighbor_fill(const float* pos, int num_atoms, const double* cell_host, const double* lo_host,
                          const double* hi_host, double rc, void* workspace, size_t workspace_bytes,
                          long num_edges, float shift_sign, int source_first, int stash_ok,
                          unsigned long long* keys, const unsigned char* target_ok, long* edge_index,
                          float* edge_shift, void* stream);

/* The search of a BATCH of structures in one pass (ABI 13, additive): `batch` [num_atoms] int64 in device memory, values
 * in [0, num_graphs), non-decreasing (the atoms of a structure are contiguous; a structure may be empty); `cells`
 * [num_graphs, 9] float32 in device memory (rows = lattice vectors), or NULL when every structure is open -- a batch is
 * all periodic or all open.  Nothing about the structures is known on the host: their atom ranges, the bounding boxes of
 * open structures and one search geometry per structure (the float64 arithmetic of the single search, with its bound of
 * 8 N_b + 64 bins per structure) are made on the device, every launch is sized by num_atoms and num_graphs alone, and no
 * pair crosses structures.  The list is the per-structure lists of the single search with the atom offsets added, in
 * the same canonical order, bit for bit.  Three calls on one workspace, as for one structure:
 *   _batch_count        -> total_device = (E, flags); flags as above (bit 3: a degenerate cell, raised for that structure
 *                          alone, which then lists no pair), plus bit 4 (value 16): `batch` decreases or leaves
 *                          [0, num_graphs) -- no pair is listed at all
 *   _batch_fill         -> the exact list after a host read of E (stash_ok / keys as for one structure)
 *   _batch_fill_padded  -> `capacity` columns, NULL edges behind the pairs, total_device rewritten with bit 2
 * target_ok masks are not part of this form.  HN_ERR_BAD_ARG, before anything is launched: a missing pointer,
 * num_graphs <= 0, rc <= 0, num_atoms * num_atoms * 4913 beyond 64 bits or 8 num_atoms + 64 num_graphs beyond 31 bits, a
 * workspace smaller than the query's for (num_atoms, num_graphs, 8); the fills also refuse num_atoms = 0.  The query
 * returns 0 for a shape the search refuses. */
size_t hermnet_neighbor_batch_workspace(int num_atoms, int num_graphs, int stash_per_atom);
int hermnet_neighbor_batch_count(const float* pos, int num_atoms, const long* batch, int num_graphs, const float* cells,
                                 double rc, void* workspace, size_t workspace_bytes, long* total_device /* [2] */,
                                 void* stream);
int hermnet_neighbor_batch_fill(int num_atoms, int num_graphs, void* workspace, size_t workspace_bytes, long num_edges,
                                float shift_sign, int source_first, int stash_ok, unsigned long long* keys,
                                long* edge_index, float* edge_shift, void* stream);
int hermnet_neighbor_batch_fill_padded(int num_atoms, int num_graphs, void* workspace, size_t workspace_bytes,
                                       long capacity, float shift_sign, int source_first, long* edge_index,
                                       float* edge_shift, long* total_device /* [2] */, void* stream);

/* ---- A13: in_subgraph (utils.py:11-24) replaced by a one-off device-side build of the relation-ordered
 * graph per neighbour list (three stable radix sorts + binary-searched row pointers, no host sync).
 * Step 1 counts the atoms of each relation (counts[T+1] device ints, last = element not in z_list);
 * the host turns the counts into the row layout `row_start[T+1]` (first row of every relation block,
 * then the first row of the unknown-element atoms) and `num_rows`; step 2 fills `out`. */
typedef struct hn_relations_out {
  int* node_order;    /* [NA]    atoms sorted by (relation, id) */
  int* row_of_node;   /* [NA]    row of every atom */
  int* z_rows;        /* [N]     atomic number per row (0 for padding rows) */
  float* row_real;    /* [N]     1 for rows that hold an atom */
  float* row_active;  /* [N]     1 for real rows of relations that receive edges (hermnet.py:56-57) */
  int* csr_rowptr;    /* [N+1] */
  int* csr_src;       /* [E]     source row, CSR order */
  int* csr_perm;      /* [E]     original edge id of each CSR edge */
  int* src_id;        /* [E]     original source / target atom ids in CSR order (edge geometry) */
  int* tgt_id;        /* [E] */
  float* shift_csr;   /* [E,3]   edge_shift in CSR order (ignored when `shift` is NULL) */
  int* csc_rowptr;    /* [T*N+1] */
  int* csc_tgt;       /* [E] */
  int* csc_pos;       /* [E] */
  int* out_rowptr;    /* [N+1]   edges by source row (position gradient); NULL (with out_edges) = not wanted */
  int* out_edges;     /* [E]     CSR positions */
} hn_relations_out;

int hermnet_relation_counts(const long* atomic_number, int num_atoms, const int* z_list, int num_rel,
                            int* counts, void* stream);
size_t hermnet_build_relations_workspace(int num_atoms, int num_rows, int num_edges, int num_rel);
/* edge_index [2,E] int64 (row 0 = source, row 1 = target, hermnet.py:135); shift [E,3] or NULL;
 * rel_active [T] bytes or NULL (NULL: a relation is active iff it receives at least one edge).
 * rows_ready != 0: `out->node_order / row_of_node / z_rows / row_real` already hold the row layout of these atomic
 * numbers (they depend on atomic_number, z_list and row_start only, not on the edges: a caller that evaluates the same
 * atoms again -- every MD step -- passes the arrays of its previous call); only the edge orders are built. */
int hermnet_build_relations(const long* atomic_number, const long* edge_index, const float* shift,
                            int num_atoms, int num_edges, const int* z_list, int num_rel,
                            const int* row_start, int num_rows, const unsigned char* rel_active,
                            const hn_relations_out* out, int rows_ready, void* workspace, size_t workspace_bytes,
                            void* stream);

/* HTNet (README.md:27 "Heterogeneous Triadic Networks"; build-defined): the relation orders of the
 * triadic graph with the same counting sort (ABI v6).  Relation (c; {p, q}) = centre element c and an unordered pair of
 * neighbour elements, T * P of them (P = T (T + 1) / 2, pairs enumerated p-major); a directed edge j -> i is listed
 * once per pair that contains element(j): E = T * num_edges entries.  SOURCE rows = the atoms in (element, id) order,
 * every element padded to `block` rows (Ns = T * block); TARGET rows = one block per relation (Nt = T * P * block).
 * Every atom must be of a listed element (the host falls back to its torch build otherwise).
 * out: node_order, row_of_node [NA], z_rows, row_real [Ns] (source rows; skipped when rows_ready), row_active [Nt],
 * csr_rowptr [Nt+1], csr_src / csr_perm (ORIGINAL edge id) / src_id / tgt_id [E], shift_csr [E,3], csc_rowptr
 * [T P Ns + 1] (groups = relation * Ns + source row), csc_tgt, csc_pos [E]; out_rowptr / out_edges unused.
 * elem_counts [T] device ints (atoms per element); tgt_row_real [Nt]; res_row [Nt] = the atom's own source row;
 * rel_active [T P] bytes or NULL (NULL: a relation is active iff it receives at least one edge HERE; an atom shard
 * passes the flags of the whole structure). */
size_t hermnet_build_triadic_workspace(int num_atoms, int num_edges, int num_elem, int block);
int hermnet_build_triadic(const long* atomic_number, const long* edge_index, const float* shift, int num_atoms,
                          int num_edges, const int* z_list, int num_elem, int block, const int* elem_counts,
                          const unsigned char* rel_active, const hn_relations_out* out, float* tgt_row_real,
                          int* res_row, int rows_ready,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- A2: HVNet.with_edge (hermnet.py:133-152) -------------------------------------------
 * edge[e] = (rx, ry, rz, d) for CSR edge e, D = pos[src] - pos[tgt] (+ shift @ cell[batch[src]]),
 * d = |D| with d ~ 0 (atol 1e-6) replaced by 1e-6, r = D / d.
 * `src_id`/`tgt_id` are ORIGINAL atom ids in CSR edge order; `shift` is [E,3] in CSR order
 * (NULL for open systems, then cell/batch are ignored); cell [B,3,3]; batch [N] original order. */
int hermnet_edge_geometry_fwd(const float* pos, const int* src_id, const int* tgt_id,
                              const float* shift, const float* cell, const int* batch,
                              int num_edges, float* edge /* [E,4] */, void* stream);

/* Backward of the above w.r.t. pos: gpos[N,3] (ORIGINAL order, overwritten) from
 * gD[E,4] (Cartesian gradient w.r.t. D, CSR order; .w ignored).  Deterministic: per-atom
 * segmented sums over `in_rowptr/in_edges` (edges whose target is the atom, sign -) and
 * `out_rowptr/out_edges` (edges whose source is the atom, sign +); both index CSR positions. */
int hermnet_edge_geometry_bwd(const float* gD, const int* in_rowptr, const int* in_edges,
                              const int* out_rowptr, const int* out_edges,
                              int num_nodes, float* gpos, void* stream);
/* The same sums with the out-edges read from the CSC order (hn_graph: csc_rowptr [T*N+1], csc_pos [E]) instead of
 * a separate out-adjacency: row a's out-edges are its T segments [csc_rowptr[t*N+a], csc_rowptr[t*N+a+1]).  Edges
 * to targets of unknown element are in no segment (they carry no message, so no gradient).  With this entry
 * point `hermnet_build_relations` may be called with out_rowptr = out_edges = NULL (one edge order fewer). */
int hermnet_edge_geometry_bwd_csc(const float* gD, const int* csr_rowptr, const int* csc_rowptr, const int* csc_pos,
                                  int num_rel, int num_nodes, float* gpos, void* stream);
/* The position gradient of either form above plus the per-atom virial (ABI 13, additive: no reference counterpart;
 * DESIGN section 1).  With D_e the edge vector exactly as hermnet_edge_geometry_fwd computes it (pos[src] - pos[tgt]
 * + shift_e @ cell[batch[src]], before the d ~ 0 clamp) and gD_e = dE/dD_e:
 *   atom_virial[a] = W_a = -1/2 sum_{e touching row a} D_e (x) gD_e   [N,9] rows, row-major [alpha][beta] = D_alpha gD_beta,
 *   unsymmetrised, energy units.  Each edge is split equally between its two atoms (the pair convention of LAMMPS and
 *   of ASE's pair calculators; the split is a convention); an edge between an atom and its own periodic image counts
 *   fully.  Summed over a graph: -sum_e D_e (x) gD_e, whose symmetric part is the virial of `virial_calc`.
 * gpos [N,3] rows is bit for bit what hermnet_edge_geometry_bwd_csc (csc_rowptr / csc_pos / num_rel given, out_rowptr =
 * out_edges = NULL) or hermnet_edge_geometry_bwd with in_edges = NULL (out_rowptr / out_edges given, csc_rowptr = csc_pos
 * = NULL, num_rel ignored) writes; every row of both outputs is written.  pos [N,3], src_id / tgt_id, shift, cell,
 * batch as for hermnet_edge_geometry_fwd (shift NULL: open system).  No atomics: bit-reproducible run to run.
 * HN_ERR_BAD_ARG: negative counts, both out-adjacencies or neither, num_rel = 0 with the CSC form, shift without
 * cell, a missing output; num_nodes = 0 is HN_OK. */
int hermnet_edge_geometry_bwd_virial(const float* gD, const int* csr_rowptr, const int* csc_rowptr, const int* csc_pos,
                                     int num_rel, const int* out_rowptr, const int* out_edges, const float* pos,
                                     const int* src_id, const int* tgt_id, const float* shift, const float* cell,
                                     const int* batch, int num_nodes, float* gpos, float* atom_virial, void* stream);
/* Per-graph virial (ABI 13, additive): graph_virial[b] = sum_{atoms i of graph b} W_i  [B,9], W_i = atom_virial[row_of_node[i]]
 * as written by the entry point above -- so graph_virial[b] = -sum_{e in b} D_e (x) gD_e, unsymmetrised, energy units; the
 * stress of graph b is -sym(graph_virial[b]) / V_b.  Rows are gathered in atom order through row_of_node [N] int64, so
 * padding rows never enter a sum.  `batch` [N] int32 (original atom order, values in [0, B)) and `graph_perm` [N] int64 =
 * the atoms sorted by graph (stable) are the pair the read-out's ordered per-graph energy sum uses: batch need not be sorted,
 * batch[graph_perm[.]] is.  graph_perm NULL: batch is already sorted; num_graphs = 1: both are ignored (every atom counts).
 * Two launches: sums of fixed chunks of 256 atoms (in graph order), then one workgroup per graph adds the chunks inside its
 * range and the atoms of its ragged ends in a fixed order -- no atomics, no memset / memcpy, no host read: bit-reproducible
 * and graph-capturable; every element of graph_virial is written (a graph without atoms gets zeros).  `workspace`: at least
 * hermnet_graph_virial_workspace bytes for num_nodes.  num_graphs = 0 or num_nodes = 0: HN_OK, nothing is launched (without
 * atoms there is no row to sum: the caller's zeros stand).  HN_ERR_BAD_ARG before any launch: a negative count, a missing
 * pointer (batch with num_graphs > 1), a workspace too small. */
size_t hermnet_graph_virial_workspace(int num_nodes);
int hermnet_graph_virial(const float* atom_virial, const long* row_of_node, const long* graph_perm, const int* batch,
                         int num_nodes, int num_graphs, void* workspace, size_t workspace_bytes, float* graph_virial,
                         void* stream);

/* ---- A3+A7(rbf_proj)+A8+A9+A10 and the residual of A6 ---------------------------------------
 * Replaces, for ALL relations of one HeteroVertexConv layer at once,
 *   PaiNNMessage.forward's rbf_proj + propagate (rmnet.py:55-73), RadialBasis.forward
 *   (rmnet.py:168-172), in_subgraph's edge slicing (utils.py:11-24) and the residual
 *   `x = (x + dx)/sqrt(2); vec = vec + dvec` (rmnet.py:24-26).
 * xh   [T,N,3H]  xh[t] = x_proj_t(LayerNorm_t(x)) for every row (sources of relation t)
 * xh_bias [T,3H] (NULL = none): added to every row of xh[t] on load, so that the x_proj GEMM can run
 *                without its broadcast bias (which would cost one more write + read of xh)
 * vec  [N,3,H]   (NULL => treated as zero: layer 0, hermnet.py:124)
 * x    [N,H]
 * wt   [T,R,3H]  rbf_proj.weight of relation t, transposed;  brbf [T,3H] its bias
 * edge [E,4]     from hermnet_edge_geometry_fwd (CSR order)
 * out: x1 [N,H], vec1 [N,3,H]; rows >= type_rowptr[T] are written as zero.
 * H must be a multiple of 64.
 * target_ranges (ABI v7; device, [T][2] int32, or NULL = every row; no reference counterpart -- atom shards, SURVEY 8(e)
 *   "run interior edges while the halo is in flight"): this launch computes only the target rows [lo_t, hi_t) of every
 *   relation t; rows outside are left untouched.  Two launches over complementary ranges give bit for bit what one
 *   launch gives: the host runs the targets whose sources are all owned rows while the halo exchange is in flight and
 *   the others behind it.  zero_unknown_rows != 0: this launch also writes the zero rows >= type_rowptr[T] (always
 *   done when target_ranges is NULL).  range_rows: the number of rows the ranges cover (host value; sizes the grid and the
 *   rows per workgroup; <= 0 = unknown, the whole row count is assumed -- correct, but a short launch then lasts as long
 *   as a full one). */
int hermnet_message_scatter_fwd(const hn_graph* g, const hn_rbf_desc* rbf, int hidden,
                                const float* xh, const float* xh_bias, const float* vec, const float* x,
                                const float* wt, const float* brbf, const float* edge,
                                float* x1, float* vec1, const int* target_ranges, int zero_unknown_rows, int range_rows,
                                void* stream);

/* Backward of hermnet_message_scatter_fwd for the force path (first order).
 * in : gx1 [N,H], gvec1 [N,3,H] (gradients w.r.t. x1, vec1) + the forward inputs
 * out: gxh [T,N,3H], gvec [N,3,H] (NULL allowed when vec was NULL), gx [N,H],
 *      gedge [H/64, E, 4]: per 64-channel column block, Cartesian gradient w.r.t. the edge
 *      vector D in CSR order (caller sums over the leading axis; buffer must be zero-filled).
 * split_t: must be 0 (HN_ERR_BAD_ARG otherwise).  The argument stays for the stable argument list; its per-relation
 *   form of the 16-lanes-per-edge backward is retired.
 * source_ranges (ABI v7; device [num_ranges][2] int32 + the same values in source_ranges_host; num_ranges = 0: every
 *   row): this launch writes gxh / gvec / gx only for the SOURCE rows of the given disjoint ascending ranges (gedge: the
 *   edges leaving those rows).  Two launches over complementary ranges give bit for bit what one gives: the host runs
 *   the halo rows first, sends their gradients home and runs the rest while they travel.  Channel-per-lane form only
 *   (edge_table given): HN_ERR_BAD_ARG otherwise.
 * gx == NULL (ABI v8; channel-per-lane form, HVNet rows, no ranges): the finishing launch is left out -- gvec_partials
 *   [T,N,3,H] keeps the per-relation sums (required then whenever vec != NULL, also for T == 1) and neither gvec nor gx is
 *   written: the consumer forms gvec = sum_t gvec_partials[t] + gvec1 and gx = gx1 / sqrt2 itself
 *   (hermnet_node_update_bwd's `pending`), or needs neither (the first layer, whose inputs carry no gradient). */
int hermnet_message_scatter_bwd(const hn_graph* g, const hn_rbf_desc* rbf, int hidden,
                                const float* xh, const float* xh_bias, const float* vec,
                                const float* wt, const float* brbf, const float* edge,
                                const float* gx1, const float* gvec1,
                                float* gxh, float* gvec, float* gx, float* gedge, int split_t,
                                const float* edge_table, float* gvec_partials,
                                const int* source_ranges, const int* source_ranges_host, int num_ranges, void* stream);

/* hermnet_message_scatter_bwd for the FIRST layer of an energy / force evaluation (ABI 13, additive): its x is the species
 * embedding, which does not depend on the positions, and it has no vec rows, so gedge is the only result anybody reads.
 * Channel-per-lane form without the source rows' sums: no gxh, no gx, no finishing launch; gedge is bit for bit what
 * hermnet_message_scatter_bwd writes for vec = NULL.  HVNet rows only (num_src = 0, res_row = NULL), edge_table required;
 * xh includes x_proj's bias (the chain kernels' form).  There is no vec argument: rows with a vec part hand gradients
 * down and take hermnet_message_scatter_bwd, which refuses a NULL gxh. */
int hermnet_message_scatter_bwd_gedge(const hn_graph* g, const hn_rbf_desc* rbf, int hidden,
                                      const float* xh, const float* wt, const float* brbf, const float* edge,
                                      const float* gx1, const float* gvec1, float* gedge,
                                      const float* edge_table, void* stream);

/* Per-edge radial record, computed ONCE per step (geometry and radial basis are shared by every layer):
 * table [E + 1, 32] floats in CSC order -- record q belongs to CSC edge q, i.e. CSR edge csc_pos[q]; `edge` stays in
 * CSR order; record E repeats record E-1, the kernel requests one record ahead without a bounds check --, so the
 * backward, which walks the CSC segments, reads one sequential stream:
 *   [2m], [2m+1]  env(u) g_m  and  (env'(u) g_m + 2 coeff env(u) g_m (u - mu_{lo+m})) / rc   for the 12 taps m of the
 *                 edge's window, g_m = exp(coeff (u - mu_{lo+m})^2): contracted with the rbf_proj rows they give
 *                 rbfh - bias and d rbfh / d d
 *   [24] padded tile row of tap 0 (int bits) | [25] the same of CSC edge q+1 | [26,27] 0 | [28..30] rhat | [31] 1/d
 * (rmnet.py:156-193 evaluated exactly as the message kernels do in registers).  When `edge_table` is handed to
 * hermnet_message_scatter_bwd (NULL = not available) the backward runs in its channel-per-lane form, which reads
 * the record through the scalar path: a wave works on one edge, its taps sit in SGPRs (csrc/message_bwd_cl.hip).
 * That form runs one workgroup per (relation, column block, row chunk) and needs `gvec_partials`, a caller-owned
 * workspace [T, N, 3, H] (per-relation partial sums of gvec, added up in a fixed order by a second small launch;
 * not needed when T = 1 or vec is NULL); without it the 16-lanes-per-edge form runs. */
int hermnet_edge_radial_table(const hn_graph* g, const hn_rbf_desc* rbf, const float* edge, float* table, void* stream);
/* The same launch, which also writes the forward's tap records (fwd_taps NULL: exactly hermnet_edge_radial_table):
 * fwd_taps [E, 16] floats in CSR order -- record e belongs to edge[e] --
 *   [0..11] g_m = exp(coeff (u - mu_{lo+m})^2), the raw taps (no envelope folded in) | [12] env(u) |
 *   [13] padded tile row of tap 0 (int bits) | [14,15] 0
 * evaluated exactly as hermnet_message_scatter_fwd evaluates them in its edge loop (same expressions, clamping and
 * operation order), once per step instead of once per layer and column block.  Every one of the E records is written;
 * the reader requests only records of edges of the row it works on, so there is no spare record behind the last. */
int hermnet_edge_radial_tables(const hn_graph* g, const hn_rbf_desc* rbf, const float* edge, float* table, float* fwd_taps,
                               void* stream);
/* hermnet_message_scatter_fwd with the taps, envelope and tile row of every edge read from `fwd_taps` (above; built from
 * the same graph, radial basis and `edge`).  Bit for bit the result of hermnet_message_scatter_fwd; fwd_taps NULL: that
 * entry point itself. */
int hermnet_message_scatter_fwd_taps(const hn_graph* g, const hn_rbf_desc* rbf, int hidden,
                                     const float* xh, const float* xh_bias, const float* vec, const float* x,
                                     const float* wt, const float* brbf, const float* edge, const float* fwd_taps,
                                     float* x1, float* vec1, const int* target_ranges, int zero_unknown_rows,
                                     int range_rows, void* stream);

/* ---- node-level fused elementwise stages (A11/A12; the GEMMs between them are library calls) ----
 * Bias convention of these stages: the GEMM in front of a stage may run WITHOUT its bias (a GEMM with a
 * broadcast bias writes and re-reads its whole output once more); the stage then adds it on load.
 * `bias` (NULL = none) is [groups, cols] for a [rows, cols] operand, group = row / rows_per_bias
 * (rows_per_bias <= 0: a single bias row) -- one group per relation block of the uniform layout.
 *
 * ScaledSiLU (rmnet.py:110-117): a = silu(h + bias)/0.6; h, a contiguous [rows, cols], cols % 4 == 0. */
int hermnet_ssilu_fwd(const float* h, const float* bias, int rows_per_bias, float* a, long rows, int cols,
                      void* stream);
/* gh[n,t,c] = g[n*g_stride_n + t*g_stride_t + c] * d ssilu(h[n,t,c] + bias); h, gh contiguous [N,T,C];
 * bias for the [N, T*C] view of h. */
int hermnet_ssilu_bwd(const float* g, const float* h, const float* bias, int rows_per_bias, float* gh,
                      int N, int T, int C, long g_stride_n, long g_stride_t, void* stream);
/* LayerNorm without affine over the last axis (`x_layernorm`, rmnet.py:52; gamma/beta are folded into the
 * following Linear by the host): n = (x - mean) * rstd, rstd = 1/sqrt(var + eps) (biased variance).
 * x, n [rows, hidden]; mean, rstd [rows]; hidden % 4 == 0, hidden <= 1024.  `hidden_real` (0 = hidden): the
 * statistics run over the first hidden_real channels only and the remaining outputs are zero -- rows of a model
 * whose hidden_channels is not a multiple of 64 are zero-padded to the next multiple for the message kernels' column
 * blocks (the reference accepts any width, hermnet.py:84-88). */
int hermnet_layernorm_fwd(const float* x, float* n, float* mean, float* rstd, int rows, int hidden, int hidden_real,
                          float eps, void* stream);
/* gx = d(n)/d(x)^T g + add  (add [rows, hidden] may be NULL; gx may alias add). */
int hermnet_layernorm_bwd(const float* g, const float* x, const float* mean, const float* rstd, const float* add,
                          float* gx, int rows, int hidden, int hidden_real, void* stream);
/* PaiNNUpdate middle (rmnet.py:95-100): vp [rows,3,2H] = vec_proj(vec1) ->
 * vdot [rows,H] = sum_d v1 v2 / sqrt(H);  xin [rows,2H] = [x1 | sqrt(sum_d v2^2 + 1e-8)]. */
int hermnet_update_mid(const float* vp, const float* x1, float* vdot, float* xin, int rows, int hidden,
                       void* stream);
/* PaiNNUpdate tail + residual (rmnet.py:101-107,29-31) + zero rows (hermnet.py:51,56-57):
 * x_out = x1 + (q1 + q2 vdot)/sqrt2, vec_out[d] = vec1[d] + q3 v1[d]; rows >= num_known or with
 * row_mask[r] == 0 (row_mask may be NULL) are written as zero without reading the other inputs. */
int hermnet_update_out(const float* q, const float* qbias /* [groups,3H] or NULL */, int rows_per_bias,
                       const float* vdot, const float* vp, const float* x1,
                       const float* vec1, const float* row_mask, float* x_out, float* vec_out,
                       int num_nodes, int num_known, int hidden, void* stream);
/* Backward of hermnet_update_out: gq [N,3H], gvdot [N,H], the v1 half of gvp [N,3,2H], and the
 * identity parts gx1 [N,H] / gvec1 [N,3,H] (masked copies of the incoming gradients). */
int hermnet_update_out_bwd(const float* gx_out, const float* gvec_out, const float* q,
                           const float* qbias, int rows_per_bias, const float* vdot,
                           const float* vp, const float* row_mask, float* gq, float* gvdot, float* gvp,
                           float* gx1, float* gvec1, int num_nodes, int num_known, int hidden, void* stream);
/* Backward of hermnet_update_mid: completes gvp (both halves) from gvdot and gxin [rows,2H] and
 * accumulates gxin[:, :H] into gx1. */
int hermnet_update_mid_bwd(const float* gvdot, const float* gxin, const float* vp, const float* xin,
                           float* gvp, float* gx1, int rows, int hidden, void* stream);

/* Energy read-out head (`out_energy`, hermnet.py:113-117,129) behind its first Linear (a library GEMM):
 * e[n] = (sum_c ScaledSiLU(h[n,c]) * w[c] + b[0]) * row_mask[n];   h [rows, cols], w [cols] = out_energy[2].weight,
 * b [1] its bias (device pointer, may be NULL), row_mask [rows] (may be NULL: all ones) zeroes padding rows. */
int hermnet_energy_head_fwd(const float* h, const float* w, const float* b, const float* row_mask, float* e,
                            int rows, int cols, void* stream);
/* gh[n,c] = ge[n] * row_mask[n] * w[c] * d ScaledSiLU(h[n,c]). */
int hermnet_energy_head_bwd(const float* ge, const float* h, const float* w, const float* row_mask, float* gh,
                            int rows, int cols, void* stream);

/* The whole read-out in one launch each way (no library GEMM): forward  h = x W0^T + b0 [rows, cols] (saved),
 * e = (w2 . ScaledSiLU(h) + b2) row_mask;  backward  gx = (ge row_mask w2 ScaledSiLU'(h)) W0  [rows, hidden].
 * w0t = out_energy[0].weight^T [hidden, cols], w0 = out_energy[0].weight [cols, hidden].  Supported: the output width
 * of each product (cols forward, hidden backward) in {64, 128, 256} and hidden * cols * 4 <= 64 KiB (the weight matrix
 * is staged in LDS); otherwise HN_ERR_BAD_ARG and the caller uses hermnet_energy_head_fwd / _bwd around its own GEMM. */
int hermnet_energy_head_fused_fwd(const float* x, const float* w0t, const float* b0, const float* w2, const float* b2,
                                  const float* row_mask, float* h, float* e, int rows, int hidden, int cols,
                                  void* stream);
int hermnet_energy_head_fused_bwd(const float* ge, const float* h, const float* w0, const float* w2,
                                  const float* row_mask, float* gx, int rows, int hidden, int cols, void* stream);

/* ABI v9: the same read-out with its H -> C product on the fp32 matrix pipe (csrc/node_chain16.hip; hidden 128, cols 64: the
 * width of BASELINE configs[1]): w0_frag16 = frag16(out_energy[0].weight [cols, hidden]), w0t_frag16 = frag16 of its transpose
 * (frag16: hermnet_node_update_fwd, "16-row form").  Same results to rounding (another summation order); ~4 us each way at
 * 10k rows where the staged-weight form above takes 24 / 16 us. */
int hermnet_energy_head16_supported(int hidden, int cols);
int hermnet_energy_head16_fwd(const float* x, const float* w0_frag16, const float* b0, const float* w2, const float* b2,
                              const float* row_mask, float* h, float* e, int rows, int hidden, int cols, void* stream);
int hermnet_energy_head16_bwd(const float* ge, const float* h, const float* w0t_frag16, const float* w2,
                              const float* row_mask, float* gx, int rows, int hidden, int cols, void* stream);

/* ---- A7 (node MLP) + A11 + A12 as chain kernels on the matrix pipe (csrc/node_chain.hip) ---------------------------------
 * One launch per chain instead of library GEMMs joined by elementwise launches; hidden activations never reach HBM.
 * hidden must be a multiple of 64 up to 512 (hermnet_node_chain_supported; other widths: the stage-wise entry points above
 * around the caller's GEMMs).  fp32 in, fp32 out, fp32 accumulation; since ABI v11 every product runs on the BF16 matrix pipe
 * as a three-way split of both operands (x = x0 + x1 + x2 exactly, bf16 planes, round to nearest even of what the planes
 * before leave; the six largest of the nine partial products, the dropped ones <= 2^-24 of a product each: fp32-equivalent at
 * 6/16 of the fp32 MFMA's pipe time).  Weights arrive split and in FRAGMENT ORDER: for an nn.Linear weight W [out, in] (or
 * its transpose for the backward products), per 32-row block cb and 16-deep k-group Q the three planes, smallest first, as
 * v_mfma_f32_32x32x16_bf16 operands -- lane l: 8 bf16 = 16 bytes --
 *     frag(W)[((cb * in/16 + Q) * 3 + s) * 64 + l] = W_(2-s)[32 cb + (l & 31)][16 Q + 8 (l >> 5) .. +7]
 * (out * in * 3 / 2 floats, 6 bytes per weight; hermnet_amd/nodeops.py: weight_fragments), so that a wave loads one coalesced
 * KiB per step straight into the operand.  `[T]` = stacked over the relations.
 *
 * hermnet_node_pre_fwd   (rmnet.py:52): for every relation t and source row,
 *     hb[t] = LayerNorm(x) W1_t^T + b1_t   (LayerNorm without affine: folded into W1 / b1 by the host; statistics over
 *                                           the first hidden_real channels, 0 = all),   saved for the backward
 *     xh[t] = ScaledSiLU(hb[t]) W2_t^T + b2_t      [T, num_src, 3H]   (bias INCLUDED: pass xh_bias = NULL to the
 *                                                                       message kernels)
 *     mean, rstd [num_src]: the LayerNorm statistics.
 *     src_ranges (device, [T][4] int32, or NULL = every row): relation t only ever gathers source rows [r0, r1) and
 *     [r2, r3) (HTNet: relation (c; p, q) gathers atoms of elements p and q); 64-row tiles outside both ranges are
 *     skipped -- their rows of hb / xh are left unwritten, their statistics must be pre-set by the caller (zeros), and
 *     the backward contributes zero for them.
 * hermnet_node_pre_bwd: gx = LayerNorm'(x)^T sum_t ((gxh[t] W2_t) * ScaledSiLU'(hb[t])) W1_t + add
 *     (w2t_frag = frag(W2_t^T [H, 3H]), w1t_frag = frag(W1_t^T [H, H]); gn_parts [T, num_src, H] is workspace; add may
 *     be NULL; gx may alias add).  gx == NULL (ABI v8): only the per-relation partial sums gn_parts are produced -- the
 *     LayerNorm backward over their sum is left to the consumer (hn_pending_grads below); x / mean / rstd / add unused.
 * row_windows (device, [num_windows][2] int32 row ranges) + window_mode (ABI v6; atom shards, no reference counterpart):
 *     0 = every row tile (row_windows may be NULL); 1 = only the tiles (hermnet_node_chain_tile_rows) that touch a window;
 *     2 = only the others.  Two calls with modes 2 and 1 on the same buffers compute what one call with mode 0 does:
 *     the host puts the halo exchange between them (forward: 2, wait + unpack, 1; backward: 1, send, 2). */
int hermnet_node_chain_supported(int hidden);   /* hidden % 64 == 0, 64 <= hidden <= 512 (the reference's default is 512) */
/* Rows per tile of the pre kernels (update = 0) or the update kernels (update != 0) at this width: 64 / 32; 0 when the
 * width is not supported.  The tiles of window modes 1 / 2 are cut at multiples of it. */
int hermnet_node_chain_tile_rows(int hidden, int update);
int hermnet_node_pre_fwd(const float* x, const float* w1_frag, const float* b1, const float* w2_frag, const float* b2,
                         float* hb, float* xh, float* mean, float* rstd, const int* src_ranges, int num_src,
                         int num_rel, int hidden, int hidden_real, float eps, const int* row_windows, int num_windows,
                         int window_mode, void* stream);
int hermnet_node_pre_bwd(const float* gxh, const float* hb, const float* w2t_frag, const float* w1t_frag,
                         float* gn_parts, const float* x, const float* mean, const float* rstd, const float* add,
                         float* gx, const int* src_ranges, int num_src, int num_rel, int hidden, int hidden_real,
                         const int* row_windows, int num_windows, int window_mode, void* stream);
/* The node projection of layer 0 in an energy / force evaluation (additive in ABI v13): there x is the species embedding, so
 * xh of a row depends on its species only.  table [num_rel, num_species, width] = xh of hermnet_node_pre_fwd run on the
 * num_species embedding rows (made once per weight refresh by the caller), width = 3 hidden, a multiple of 4;
 *     xh[t][r][:] = table[t][z_rows[r]][:]      for every relation t and all num_rows rows (z_rows int64; a value outside
 *                                               [0, num_species) is clamped into it),
 * the bits hermnet_node_pre_fwd writes for x[r] = embedding[z_rows[r]].  No hb / mean / rstd: nothing below layer 0 takes a
 * gradient.  Arrays of 4 GiB and more are handled (64-bit indices). */
int hermnet_species_expand(const float* table, const long* z_rows, float* xh, int num_rows, int num_rel, int num_species,
                           int width, void* stream);
/* hermnet_node_update_fwd (rmnet.py:94-107, 29-31; hermnet.py:51,56-61), target rows in relation order:
 *     vp = vec1 Wv^T  [N,3,2H] = (v1 | v2), saved;   vdot = sum_d v1 v2 / sqrt(H);   n = sqrt(sum_d v2^2 + 1e-8) -> nrm
 *                                                                                    [N,H], saved
 *     h2b = [x1 | n] Wx0^T + bx0  [N,H], saved;      (p | q | r) = ScaledSiLU(h2b) Wx2^T + bx2;   q23 = (q | r) [N,2H], saved
 *     x_out = x1 + (p + q vdot)/sqrt2,  vec_out[d] = vec1[d] + r v1[d];   rows with row_active == 0 (row_active may be
 *     NULL: all active) and rows >= type_rowptr[T] are written as zero.
 * type_rowptr [T+1] on the device and the same values on the host (`type_rowptr_host`: the launch geometry).
 * hermnet_node_update_bwd: (gx_out, gvec_out) -> (gx1, gvec1), the gradients w.r.t. x1 / vec1 (parameters are
 *     constants); wx2t_frag = frag(Wx2^T [H,3H]), wx0t_frag = frag(Wx0^T [2H,H]), wvt_frag = frag(Wv^T [H,2H]).
 * tile_rows (ABI v7): 0 = the width's default row tile (32; 64 at hidden 64); 16 = the 16-row form (hidden 128 only:
 *     v_mfma_f32_16x16x32_bf16, csrc/node_chain16.hip) -- every *_frag argument must then be the frag16 copy of the weight,
 *     frag16(W)[((b * K/32 + Q) * 3 + s) * 64 + l] = 8 bf16 W_(2-s)[16 b + (l & 15)][32 Q + 8 (l >> 4) .. +7]
 *     (nodeops.weight_fragments16).
 *     hermnet_node_update_tile_rows says which form shortens the launch for a row layout (small grids: 32-row tiles
 *     leave most CUs with one workgroup while a few get two; 16-row tiles cost twice the weight bytes from L2).
 * pending (ABI v8; may be NULL): the incoming gradients of this layer's outputs have not been formed yet -- they still sit
 *     in the partial sums of the layer above, which skipped its two small finishing launches (hermnet_message_scatter_bwd
 *     and hermnet_node_pre_bwd, each called with gx == NULL).  The update backward then forms them for the rows of each of
 *     its tiles first, with the same operations in the same order (bit-identical to the separate launches),
 *         gx_out[r]   = LayerNorm'(x[r])^T (sum_p gn_parts[p][r]) + gx1[r] / sqrt2
 *         gvec_out[r] = sum_p gvec_parts[p][r] + gvec1[r]             (the "+" terms on rows < type_rowptr[T] only),
 *     WRITES them to gx_out / gvec_out (buffers of the caller; the `const` is nominal in this mode) and goes on as usual.
 *     Needs num_src == num_nodes (HVNet rows) in the layer above.  Saves two launches per layer boundary. */
typedef struct hn_pending_grads {
  const float* gn_parts;    /* [num_parts][num_nodes][hidden]     from hermnet_node_pre_bwd(gx = NULL) */
  const float* gvec_parts;  /* [num_parts][num_nodes][3][hidden]  from hermnet_message_scatter_bwd(gx = NULL) */
  const float* x;           /* [num_nodes][hidden]  the layer above's input, mean / rstd [num_nodes] its LayerNorm statistics */
  const float* mean;
  const float* rstd;
  const float* gx1;         /* [num_nodes][hidden], [num_nodes][3][hidden]: the layer above's update-backward results */
  const float* gvec1;
  int num_parts;            /* the relations T of the layer above */
  int hidden_real;          /* as in hermnet_node_pre_bwd (0 = hidden) */
  /* ABI v9, fused form (tile_rows == 16 only; gn_parts is then unused and may be NULL): the layer above did not run
   * hermnet_node_pre_bwd at all -- the update backward runs that chain for the rows of each of its tiles first,
   *     gn_t = ((gxh[t] W2_t) * ScaledSiLU'(hb[t])) W1_t,   sum_t in registers in the order (gn_0 + gn_1) + gn_2 ...,
   * then the LayerNorm backward on the tile: no [T, num_nodes, hidden] partial sums in memory, one launch less per layer
   * boundary.  Bit-identical to hermnet_node_pre_bwd16 followed by the `gn_parts` form. */
  const float* gxh;         /* [num_parts][num_nodes][3 hidden]  from hermnet_message_scatter_bwd (NULL: the gn_parts form) */
  const float* hb;          /* [num_parts][num_nodes][hidden]    saved by the layer above's node projection */
  const float* w2t_frag16;  /* [num_parts] frag16(W2_t^T [hidden, 3 hidden]), frag16(W1_t^T [hidden, hidden]) of the layer above */
  const float* w1t_frag16;
} hn_pending_grads;
int hermnet_node_update_tile_rows(const int* type_rowptr_host, int num_nodes, int num_rel, int hidden);
int hermnet_node_update_fwd(const float* x1, const float* vec1, const float* wv_frag, const float* wx0_frag,
                            const float* bx0, const float* wx2_frag, const float* bx2, const float* row_active,
                            const int* type_rowptr, const int* type_rowptr_host, float* vp, float* h2b, float* q23,
                            float* nrm, float* x_out, float* vec_out, int num_nodes, int num_rel, int hidden,
                            int tile_rows, void* stream);
int hermnet_node_update_bwd(const float* gx_out, const float* gvec_out, const float* vp, const float* h2b,
                            const float* q23, const float* nrm, const float* wx2t_frag, const float* wx0t_frag,
                            const float* wvt_frag,
                            const float* row_active, const int* type_rowptr, const int* type_rowptr_host, float* gx1,
                            float* gvec1, int num_nodes, int num_rel, int hidden, int tile_rows,
                            const hn_pending_grads* pending, void* stream);
/* hermnet_node_update_bwd_held (ABI 13, additive): hermnet_node_update_bwd for a caller that never reads gvec_out.  Requires
 * `pending` in its gn_parts form (pending->gxh == NULL), tile_rows == 16 and hidden 128 (frag16 weights): HN_ERR_BAD_ARG before
 * any launch otherwise.  The gvec sums the launch forms from the partial sums go from registers and LDS straight into the
 * products: gvec_out is neither read nor written and may be NULL; gx_out is workspace of the launch (written, then read back by
 * it).  gx1, gvec1: bit for bit what hermnet_node_update_bwd returns for the same arguments. */
int hermnet_node_update_bwd_held(const float* gx_out, const float* gvec_out, const float* vp, const float* h2b,
                                 const float* q23, const float* nrm, const float* wx2t_frag16, const float* wx0t_frag16,
                                 const float* wvt_frag16,
                                 const float* row_active, const int* type_rowptr, const int* type_rowptr_host, float* gx1,
                                 float* gvec1, int num_nodes, int num_rel, int hidden, int tile_rows,
                                 const hn_pending_grads* pending, void* stream);

/* The LAST layer of an energy / force evaluation (ABI 13, additive; hidden 128, 16-row tiles, frag16 weights): the read-out
 * takes x only, so vec_out feeds nothing and its gradient is identically zero.
 * hermnet_node_update_fwd_last: hermnet_node_update_fwd (16-row form) without vec_out -- the r third of the last product and
 *   dvec = r v1 are not computed; x_out, vp, h2b, nrm and the q half of q23 [N, 2H] are bit for bit the general form's, the r
 *   half of q23 is left unwritten.
 * hermnet_node_update_bwd_last: hermnet_node_update_bwd (16-row form) for gvec_out = 0, which is not passed; reads the q half
 *   of q23 only.  gx1, gvec1: bit for bit the general form's results for an all-zero gvec_out, given finite saved tensors
 *   and no partial sum that underflows to -0 (products below ~1e-45): there the two forms may differ in the SIGN of a zero.
 *   `pending` must be NULL (no layer above the last one hands anything down): HN_ERR_BAD_ARG otherwise. */
int hermnet_node_update_fwd_last(const float* x1, const float* vec1, const float* wv_frag16, const float* wx0_frag16,
                                 const float* bx0, const float* wx2_frag16, const float* bx2, const float* row_active,
                                 const int* type_rowptr, const int* type_rowptr_host, float* vp, float* h2b, float* q23,
                                 float* nrm, float* x_out, int num_nodes, int num_rel, int hidden, void* stream);
int hermnet_node_update_bwd_last(const float* gx_out, const float* vp, const float* h2b, const float* q23,
                                 const float* nrm, const float* wx2t_frag16, const float* wx0t_frag16,
                                 const float* wvt_frag16, const float* row_active, const int* type_rowptr,
                                 const int* type_rowptr_host, float* gx1, float* gvec1, int num_nodes, int num_rel,
                                 int hidden, const hn_pending_grads* pending, void* stream);

/* ---- ABI v9: one node launch per layer boundary, each way (csrc/node_chain16.hip; hidden 128, 16-row tiles).
 * A tile's PaiNNUpdate of layer l (rmnet.py:94-107, 29-31) and the node projection of layer l + 1 on the rows it has just
 * produced (rmnet.py:52 for every relation of the NEXT layer) are row-local: hermnet_node_update_pre_fwd runs both in one
 * launch -- the arguments of hermnet_node_update_fwd (16-row form: frag16 weights) followed by those of the next layer's
 * projection (w1_frag16 = frag16 of [next_num_rel] W1 with the LayerNorm affine folded in, b1, w2_frag16, b2; outputs hb, xh,
 * mean, rstd as hermnet_node_pre_fwd writes them, for all num_nodes rows).  The backward mirror is hermnet_node_update_bwd with
 * pending->gxh set.  hermnet_node_pre_fwd16 / hermnet_node_pre_bwd16 run the same projection phases as kernels of their own
 * (16-row tiles, frag16 weights; pre_bwd16 writes the per-relation partial sums gn_parts only): update_fwd(tile_rows = 16) +
 * pre_fwd16 is bit-identical to update_pre_fwd, pre_bwd16 + update_bwd(pending->gn_parts) to update_bwd(pending->gxh). */
int hermnet_node_fused_supported(int hidden);
int hermnet_node_update_pre_fwd(const float* x1, const float* vec1, const float* wv_frag16, const float* wx0_frag16,
                                const float* bx0, const float* wx2_frag16, const float* bx2, const float* row_active,
                                const int* type_rowptr, const int* type_rowptr_host, float* vp, float* h2b, float* q23,
                                float* nrm, float* x_out, float* vec_out, int num_nodes, int num_rel, int hidden,
                                const float* w1_frag16, const float* b1, const float* w2_frag16, const float* b2, float* hb,
                                float* xh, float* mean, float* rstd, int next_num_rel, int hidden_real, float eps,
                                void* stream);
int hermnet_node_pre_fwd16(const float* x, const float* w1_frag16, const float* b1, const float* w2_frag16, const float* b2,
                           float* hb, float* xh, float* mean, float* rstd, int num_src, int num_rel, int hidden,
                           int hidden_real, float eps, void* stream);
int hermnet_node_pre_bwd16(const float* gxh, const float* hb, const float* w2t_frag16, const float* w1t_frag16,
                           float* gn_parts, int num_src, int num_rel, int hidden, void* stream);

/* HTNet (hermnet.py:155-157 is a stub; DESIGN.md "HTNet"): a centre atom's P pair relations are averaged.  Target rows
 * are [num_elem][pairs][block] blocks of `block` rows ("virtual" rows, one per atom and pair relation):
 *   mode 0:  x_out [rows_out,H], vec_out [rows_out,3,H]: row c*block + i = scale * sum_k in[(c*pairs + k)*block + i]
 *            (scale_x for x, scale_vec for vec; the mean: 1/pairs), rows >= num_elem*block are written as zero (atoms
 *            of elements outside `elems`, hermnet.py:51)
 *   mode 1:  x_out / vec_out [num_elem*pairs*block, ...] = the gradient w.r.t. the virtual rows: scale * in[c*block + i]
 *            (x_in / vec_in then hold the [rows_out, ...] gradient)
 *   mode 2:  as mode 0 for the rows < num_elem*block, ACCUMULATED into x_out / vec_out (the residual's gradient summed
 *            over a centre's virtual rows: scale_x = 1/sqrt(2), scale_vec = 1, rmnet.py:24-26).  row_ranges (ABI v7;
 *            device [num_ranges][2] int32, 0 = every row; mode 2 only): only the output rows of these ranges (atom
 *            shards: the message backward runs in two launches over complementary source-row ranges). */
int hermnet_pair_mean(int mode, const float* x_in, const float* vec_in, float* x_out, float* vec_out, int num_elem,
                      int pairs, int block, int rows_out, int hidden, float scale_x, float scale_vec,
                      const int* row_ranges, int num_ranges, void* stream);

/* ---- the training step's per-edge message algebra (rmnet.py:58-66 inside example/dist_train.py:86-99, where the
 * forces are differentiated w.r.t. the parameters: every op needs a second derivative).  ABI v6; csrc/train_kernels.hip.
 *   X [E,3H] = x_proj(LayerNorm(x)) of the edge's source (Xs | Xa | Xb),  R [E,3H] = rbf_proj(rbf(d)) (Rs | Ra | Rb, the
 *   constant factors 1/sqrt(3H), 1/sqrt(H) already on the a / b parts),  V [E,3,H] = vec of the source or NULL (layer 0),
 *   U [E,3] = rhat.   hidden must be a multiple of 4.
 *   fwd :  S = Xs Rs [E,H];  M_d = (Xb Rb) U_d + V_d (Xa Ra) [E,3,H]        (their row sums are dx, dvec)
 *   bwd :  cotangents (GS, GM) -> gX, gR [E,3H], gV [E,3,H] (NULL with V), gU [E,3]
 *   bwd2:  cotangents (cX, cR, cV, cU; each may be NULL = zero) of bwd's outputs -> dGS [E,H], dGM [E,3,H], dX, dR
 *          [E,3H], dV [E,3,H] (NULL with V), dU [E,3]   -- the backward of the backward; the map is multilinear, so all
 *          three are per-edge products and channel sums (deterministic, no atomics).
 *   x_rows / v_rows / t_rows [E] int64 (each may be NULL = row e): X and cX are read at row x_rows[e] of their arrays
 *   (x_j = xh[(relation, source)] without a gathered copy), V and cV at v_rows[e] (vec[source]), GS and GM at t_rows[e]
 *   (the cotangents of dx, dvec of the edge's target); R and cR at r_rows[e], where gR / dR are written as well (R kept
 *   in another edge order; rows no edge points to are left untouched); every other OUTPUT is per edge -- the caller
 *   sums gX / gV / dGS / ... into rows with hermnet_segment_sum. */
int hermnet_edge_message_fwd(const float* X, const float* R, const float* V, const float* U, long num_edges, int hidden,
                             const long* x_rows, const long* v_rows, const long* r_rows, float* S, float* M,
                             void* stream);
int hermnet_edge_message_bwd(const float* GS, const float* GM, const float* X, const float* R, const float* V,
                             const float* U, long num_edges, int hidden, const long* x_rows, const long* v_rows,
                             const long* t_rows, const long* r_rows, float* gX, float* gR, float* gV, float* gU,
                             void* stream);
int hermnet_edge_message_bwd2(const float* cX, const float* cR, const float* cV, const float* cU, const float* GS,
                              const float* GM, const float* X, const float* R, const float* V, const float* U,
                              long num_edges, int hidden, const long* x_rows, const long* v_rows, const long* t_rows,
                              const long* r_rows, float* dGS, float* dGM, float* dX, float* dR, float* dV, float* dU,
                              void* stream);

/* Segmented row sum with an optional gather (the adjoint of a row gather; training path, ABI v6):
 * out[r] = sum over q in [rowptr[r], rowptr[r+1]) of x[perm ? perm[q] : q], rows of `width` floats (a multiple of 4),
 * members added in list order (deterministic).  perm [rowptr[num_rows]] int64 or NULL; rowptr [num_rows + 1] int64. */
/* The same three kernels with the ROW SUMS inside (ABI v8): one lane group per output row of a grouping of the edges --
 * group g holds the edges group_edges[q] (q itself when group_edges is NULL), q in [group_rowptr[g], group_rowptr[g+1]) --
 * and whatever is summed over that grouping never reaches HBM per edge.  fwd: groups = target rows, dx [G,H] and dv [G,3,H]
 * are the sums of S and M.  bwd / bwd2: groups = the (relation, source) rows of xh: gX_rows / dX_rows [G,3H] are the sums,
 * gV_rows / dV_rows [G,3,H] the per-group partial sums (the caller adds a source's T groups); gR, gU, dGS, dGM, dR, dU stay
 * per edge as in the kernels above.  Edges in no group are not visited. */
int hermnet_edge_message_fwd_rows(const float* X, const float* R, const float* V, const float* U, long num_edges, int hidden,
                                  const long* x_rows, const long* v_rows, const long* r_rows, const long* group_rowptr,
                                  const long* group_edges, long num_groups, float* dx, float* dv, void* stream);
int hermnet_edge_message_bwd_rows(const float* GS, const float* GM, const float* X, const float* R, const float* V,
                                  const float* U, long num_edges, int hidden, const long* x_rows, const long* v_rows,
                                  const long* t_rows, const long* r_rows, const long* group_rowptr, const long* group_edges,
                                  long num_groups, float* gX_rows, float* gR, float* gV_rows, float* gU, void* stream);
int hermnet_edge_message_bwd2_rows(const float* cX, const float* cR, const float* cV, const float* cU, const float* GS,
                                   const float* GM, const float* X, const float* R, const float* V, const float* U,
                                   long num_edges, int hidden, const long* x_rows, const long* v_rows, const long* t_rows,
                                   const long* r_rows, const long* group_rowptr, const long* group_edges, long num_groups,
                                   float* dGS, float* dGM, float* dX_rows, float* dR, float* dV_rows, float* dU,
                                   void* stream);
int hermnet_segment_sum(const float* x, const long* perm, const long* rowptr, long num_rows, int width, float* out,
                        void* stream);

/* Node-level stages of the TRAINING step (train() mode; no reference counterpart beyond the formulas: rmnet.py:52, 94-107,
 * 110-117, differentiated twice by autograd there).  ONE entry point, twelve kernels (csrc/train_node_kernels.hip); `in` / `out`
 * are host arrays of device pointers, rows x hidden fp32 row-major unless noted, hidden % 4 == 0, hidden <= 1024.
 * Stages:  SILU y = x sigmoid(x);  LN y = LayerNorm(x) without affine, eps = c0;
 *          MID (vp [R,3,2H] = (v1 | v2), xt) -> vdot = c0 sum_d v1 v2, xin [R,2H] = (xt | sqrt(sum_d v2^2 + c1));
 *          OUT (q [R,3H] = (q1|q2|q3), vdot, vp, xt, vt [R,3,H], m [R] or NULL) -> xo = m (xt + (q1 + q2 vdot) c0), vo_d = m (vt_d + q3 v1_d).
 * `bwd` maps the cotangents of a stage's outputs to those of its inputs, `bwd2` does the same for `bwd` itself.
 *  op  kernel     in                                                                   out
 *   1  silu_bwd   gy, x                 (rows = number of float4 elements)              gx
 *   2  silu_bwd2  u (cot. of gx), gy, x                                                 c_gy, c_x
 *   3  mid_fwd    vp, xt                                                                vdot, xin
 *   4  mid_bwd    g_vdot, g_xin, vp                                                     g_vp, g_xt
 *   5  mid_bwd2   u_vp*, u_xt*, g_vdot, g_xin, vp                                       c_gvdot, c_gxin, c_vp
 *   6  out_fwd    q, vdot, vp, xt, vt, m*                                               xo, vo
 *   7  out_bwd    gx, gv, q, vdot, vp, m*                                               g_q, g_vdot, g_vp, g_xt*, g_vt*
 *   8  out_bwd2   c_gq*, c_gvdot*, c_gvp*, c_gxt*, c_gvt*, gx, gv, q, vdot, vp, m*      d_gx, d_gv, d_q, d_vdot, d_vp
 *   9  ln_bwd     gy, x                                                                 gx
 *  10  ln_bwd2    v (cot. of gx), gy, x                                                 c_gy, c_x
 *  11  res_fwd    x, dx, v* [R,3,H], dv, m*    (rmnet.py:24-26: x1 = m c0 (x + dx), v1 = m (v + dv))   x1, v1
 *  12  mask_scale g1*, gv1*, m*   (its backward, for both summands, and its own backward)         m c0 g1, m gv1
 * (* = may be NULL: a zero cotangent / no mask / an output nobody reads).  num_in / num_out must be the counts above. */
int hermnet_train_node_op(int op, const float* const* in, int num_in, float* const* out, int num_out, long rows, int hidden,
                          float c0, float c1, void* stream);

/* Halo exchange packing for atom-sharded runs (one process per GPU; the exchange itself is an RCCL all-to-all made
 * by the host code, hermnet_amd/sharding.py).  A packed row = [ x (H) | vec (3H) ]; idx [n] (int64) holds rows.
 *   mode 0  buf[k] = rows[idx[k]]                         pack what the neighbours need
 *   mode 1  buf[k] = rows[idx[k]]; rows[idx[k]] = 0       pack the gradients of my halo rows and clear them
 *   mode 2  rows[idx[k]] = buf[k]                         unpack received halo rows (idx unique)
 * Any other mode: HN_ERR_BAD_ARG (the float-atomic accumulate of ABI <= 6 is gone: hermnet_halo_accumulate). */
int hermnet_halo_rows(int mode, float* x, float* vec, const long* idx, int n, int hidden, float* buf, void* stream);

/* Accumulating returned gradients at their owner: the returned packed rows are summed per owner row in
 * a FIXED order, rows[seg_rows[u]] += sum_{q in [seg_ptr[u], seg_ptr[u+1])} buf[seg_pos[q]]  (seg_rows unique, int64
 * lists prepared once per exchange plan by hermnet_amd/sharding.py) -- no atomics, bit-reproducible. */
int hermnet_halo_accumulate(float* x, float* vec, const long* seg_rows, const long* seg_ptr, const long* seg_pos,
                            int num_rows, int hidden, const float* buf, void* stream);

/* Halo exchange of PROJECTED rows (ABI v12; the default form of the per-layer exchange where the node chain kernels run:
 * hermnet_amd/layer.py).  What a neighbour needs of a halo atom is xh[t] = x_proj_t(LayerNorm(x)) for every relation
 * (rmnet.py:52: the source rows the message gathers, rmnet.py:58) and vec: T + 1 blocks of `width` = 3H floats.  The owner
 * sends those -- 12H floats per atom instead of 4H -- and the receiver runs NO node projection on halo rows, forward or
 * backward (no windowed second launch of the chain kernels, no finishing launches in front of the gradient exchange).
 * A packed row = [ a[0][r] | ... | a[S-1][r] | sum_{s < num_sum} b[s][r] ], a[j] = a + j * a_seg_stride, b[s] = b + s *
 * b_slice_stride, rows `width` floats apart.  Forward: a = xh [T, N, 3H], b = vec (num_sum 1).  Backward: a = gxh, b = the
 * per-relation partial sums of gvec [T, N, 3, H] (num_sum T: summed, ascending relation, while they are packed).
 *   mode 0 pack;  mode 1 pack, then clear every source;  mode 2 unpack (a[j][r] = block j, b[0][r] = block S; idx unique) */
int hermnet_halo_proj_rows(int mode, float* a, long a_seg_stride, int num_seg, float* b, long b_slice_stride, int num_sum,
                           const long* idx, int n, int width, float* buf, void* stream);
/* ... and the owner's side of the return path: a[j][seg_rows[u]] += sum of block j of the returned rows of segment u,
 * b[seg_rows[u]] += the sum of their last blocks, in list order (lists as for hermnet_halo_accumulate): no atomics. */
int hermnet_halo_proj_accumulate(float* a, long a_seg_stride, int num_seg, float* b, const long* seg_rows, const long* seg_ptr,
                                 const long* seg_pos, int num_rows, int width, const float* buf, void* stream);

/* float4 stream copy dst[i] = src[i] (16-byte aligned pointers, num_floats % 4 == 0): not part of the path -- the yardstick
 * for SURVEY.md 8(d)'s "measured copy bandwidth on the box" (bench.py: roofline.measured_copy_GBps; the method of
 * MI355X_MICROARCH.md's 6.29 TB/s figure).  `workgroups` <= 0: 8 per CU. */
int hermnet_stream_copy(const float* src, float* dst, size_t num_floats, int workgroups, void* stream);

/* Parameter guard (ABI v9).  The host side caches kernel-ready copies of the module's parameters and rebuilds them when a
 * parameter's identity / version / address changes; a write through `.data` changes none of these (the reference has no such
 * cache: /root/reference/HermNet/hermnet.py:118-131 reads nn.Parameters directly on every call).  `tensor_ptrs` [n] device array
 * of device pointers to CHUNKS of the parameter tensors (at most 4096 32-bit words each: one workgroup per chunk),
 * `word_counts` [n] their sizes in words, `fingerprints` [n] uint32.
 * check == 0: record a position-weighted wrapping sum of every tensor's words.  check != 0: compare; on any difference
 * flag[0] = 1 and, if `poison` is given, poison[0] = NaN (the caller passes a cached value every result depends on, so a step on
 * stale copies yields NaN instead of the old numbers).  One launch, no host read. */
int hermnet_param_guard(const void* const* tensor_ptrs, const long* word_counts, int num_tensors, unsigned* fingerprints,
                        int check, float* poison, int* flag, void* stream);

/* Per-step flags of an atom-sharded step in two launches (clear + mark; ABI v10; hermnet_amd/sharding.py: slab_data,
 * plan_moved -- sixteen elementwise / index launches before).  The reference skips a relation when no atom of its element receives an edge anywhere
 * in the structure (/root/reference/HermNet/hermnet.py:56-57): every rank marks the (target element, source element) pairs its
 * own list joins and the ranks reduce the table.  `edge_index` [2, columns] (rows: source, target; NULL edges of a padded list
 * = -1), `atomic_number` [num_atoms] of the LOCAL atoms, `total` [2] = (pairs found, flags) of a padded list or null,
 * `capacity` its columns.  `has_in` [128 * 128 + 3] int32 is zeroed here, then: [zt * 128 + zs] = 1 per joined pair (elements
 * clamped to 127), [128 * 128] = 1 if the list holds NULL edges, [128 * 128 + 1] = 1 if the padded list is incomplete
 * (flags != 0 or more pairs than columns), [128 * 128 + 2] = 1 if an atom of `pos` [num_pos, 3] is further than
 * sqrt(max_dist2) from its position in `pos_ref` (num_pos = 0: not asked).  No host read, no memset node. */
int hermnet_shard_step_flags(const long* edge_index, long columns, const long* atomic_number, int num_atoms, const long* total,
                             long capacity, int* has_in, const float* pos, const float* pos_ref, long num_pos, float max_dist2,
                             void* stream);

/* rbf_proj of the TRAINING path on the bucketed basis (ABI v13; hermnet_amd/trainops.py: BucketedBasis, BandP / BandQ / BandS;
 * /root/reference/HermNet/rmnet.py:55 on 32-centre windows, differentiated twice by /root/reference/example/dist_train.py:86-99).
 * Edges sorted by (relation, distance bucket) form `num_chunks` chunks of `rows_per_chunk` rows (a multiple of 32; _grad_b: of
 * 16); a chunk has ONE 32 x width weight window (width = 3 * hidden: a multiple of 32, at most 480).  Exact fp32 products on the
 * fp32 matrix pipe, fixed summation order.
 *   hermnet_band_product          out[c] = a[c] b[c] + bias[c]       a [nc,C,32]  b [nc,32,width]  bias [nc,width] | NULL  out [nc,C,width]
 *   hermnet_band_product_grad_a   ga[c]  = (g1[c] + g2[c]) b[c]^T     g1, g2 [nc,C,width] (g2 NULL = absent)               ga  [nc,C,32]
 *   hermnet_band_product_grad_b   gb[c]  = a[c]^T (g1[c] + g2[c]),  gbias[c] = column sums of g1[c] + g2[c] (gbias NULL = not asked)
 *   hermnet_band_product_grads    ga, gb and gbias of the two above from ONE pass over g1 (+ g2) (a, b, g1, ga, gb required)
 * g1 + g2: the radial array has two consumers in the autograd graph (the message algebra and its backward); their gradients are
 * added while they are read.  hermnet_band_product_supported: 1 when (rows_per_chunk, width) is a shape these kernels take. */
int hermnet_band_product_supported(int rows_per_chunk, int width);
int hermnet_band_product(const float* a, const float* b, const float* bias, long num_chunks, int rows_per_chunk, int width,
                         float* out, void* stream);
int hermnet_band_product_grad_a(const float* g1, const float* g2, const float* b, long num_chunks, int rows_per_chunk, int width,
                                float* ga, void* stream);
int hermnet_band_product_grad_b(const float* a, const float* g1, const float* g2, long num_chunks, int rows_per_chunk, int width,
                                float* gb, float* gbias, void* stream);
int hermnet_band_product_grads(const float* a, const float* b, const float* g1, const float* g2, long num_chunks,
                               int rows_per_chunk, int width, float* ga, float* gb, float* gbias, void* stream);
/* Column sums of x [num_slices, rows, width] over the rows (ABI v13; the bias gradients of the training path's node linears,
 * /root/reference/HermNet/rmnet.py:52,94-100): partial [num_slices, ceil(rows / rows_per_block), width] holds one sum per block of
 * rows; the caller adds the partials (fixed order).  width a multiple of 4, at most 1024. */
int hermnet_col_sum(const float* x, long num_slices, long rows, int width, int rows_per_block, float* partial, void* stream);

/* Edge unit vectors and their two derivatives for the training path (ABI v13; /root/reference/HermNet/hermnet.py:144-152 with the
 * distance floor of :146-147): D [E,3] -> U = D / d, d = max(|D|, 1e-6).
 *   order 0: out0 = U [E,3], out1 = d [E];   order 1: out0 = gD [E,3] from the cotangents gU [E,3]*, gd [E]*;
 *   order 2: (cotangent C [E,3] of gD) out0 = c_gU [E,3], out1 = c_gd [E], out2 = c_D [E,3].      (* = may be NULL: zero) */
int hermnet_edge_unit(int order, const float* D, const float* gU, const float* gd, const float* C, long num_edges, float* out0,
                      float* out1, float* out2, void* stream);

/* The basis window of the bucketed rbf_proj and its two derivatives (ABI v13; /root/reference/HermNet/rmnet.py:168-193 on the 32
 * centres of a chunk): phi[r][k] = w[c][k] e(u_r) exp(coeff (u_r - mu[c][k])^2), c = r / rows_per_chunk, e = the polynomial
 * envelope of exponent env_p for u < 1 on rows with src[r] < num_edges (rows that hold an edge), 0 otherwise.
 *   order 0: out0 = phi [rows,32];   order 1: out0 = g_u [rows] = sum_k g[r][k] dphi/du  (g [rows,32]);
 *   order 2: out0 = d_g [rows,32] = cu[r] dphi/du, out1 = d_u [rows] = cu[r] sum_k g[r][k] d2phi/du2  (cu [rows]).
 * mu, w [num_chunks,32]: centres and column weights (0 for centres outside the basis). */
int hermnet_basis_window(int order, const float* u, const long* src, long num_edges, const float* mu, const float* w,
                         long num_chunks, int rows_per_chunk, float coeff, int env_p, const float* g, const float* cu, float* out0,
                         float* out1, void* stream);

/* Host-side (CPU) evaluation of the per-edge radial contraction exactly as the device code
 * computes it (banded 12-tap Gaussian window): rb[c] = b[c] + env(u) * sum_k W[c,k] g_k(u) and
 * its derivative d rb / d d.  Used by the CPU test-suite to check the banded formulation
 * against the dense reference formula without a GPU.  All pointers are HOST pointers. */
int hermnet_host_rbf_row(const float* offset_host, int num_rbf, float inv_rc, float coeff,
                         int env_kind, int env_p, const float* wt_host /* [R,C] */,
                         const float* b_host /* [C] */, int C, float d,
                         float* rb_host /* [C] */, float* drb_host /* [C] */);

/* Host-side (CPU) probe of the neighbour search's cell-list geometry: the ONE routine that hermnet_neighbor_count /
 * _fill run on the host and that the device-cell and batch forms run in a kernel (csrc/neighbor_kernels.hip,
 * nbr_make_geom), so that its arithmetic can be checked without a GPU.  cell_host: 9 doubles (rows = lattice vectors), or
 * NULL with the corners lo_host / hi_host [3] of an open structure's bounding box; num_atoms >= 1 bounds the grid (at most
 * 8 num_atoms + 64 bins).  geom_host [22] = cell [9] | inverse [9] | lo [3] | rc^2; grid_host [7] = nbins [3] | reach [3] |
 * periodic.  HN_ERR_BAD_ARG: a missing pointer, rc <= 0, num_atoms < 1, or a degenerate geometry -- a singular cell, one so
 * small that the cutoff reaches beyond 8 bins, a cell or box that is not finite (the search's host form once sent the
 * latter through an undefined cast; it refuses them now).  All pointers are HOST pointers. */
int hermnet_host_neighbor_geometry(const double* cell_host, const double* lo_host, const double* hi_host, double rc,
                                   int num_atoms, double* geom_host /* [22] */, int* grid_host /* [7] */);

/* Device-resident MD (added within ABI v13: new entry points only; hermnet_amd/md.py: DeviceMD; csrc/md_kernels.hip, md_step.h).
 * The reference leaves dynamics to ASE on the host (/root/reference/HermNet/plugin/ase_interface/calculator.py:49: one
 * list + model call per step).  Here hermnet_md_advance is enqueued in FRONT of the captured neighbour search and
 * hermnet_md_finish BEHIND the force backward, so that one replay of the step's hipGraph is one time step and nothing is
 * read or written by the host in between.  Units: eV, Angstrom, fs; masses enter through the caller's coefficients only.
 *
 * Caller-owned state (all allocated outside the capture):
 *   x, v, x0, v0 [N,3] float64  coordinates / velocities and their start-of-step backup;   f_prev [N,3] float32 the last
 *   accepted forces (the step's own force output does not exist when advance is recorded);   image, image0 [N,3] int32
 *   lattice vectors removed by wrapping (x + image cell = the unwrapped path) and their backup;   kick [N] = dt / (2 m_i);
 *   half_mass [N] = m_i / 2 (0 for an atom that is held);   c1 [B], sigma [N] the Langevin coefficients exp(-friction dt)
 *   and sqrt(kB T (1 - c1^2) / m_i);   batch [N] int64 non-decreasing or NULL (one graph), graph_ptr [B+1] int32 its atom
 *   ranges;   cell [B,9] float32 -- the tensor the search reads -- and inv_cell [B,9] float64 its inverse (made once on the
 *   host: the kernels only add, multiply and floor);   pos32 [N,3] float32 the captured coordinate input of the model;
 *   ke_atom [N] float64 scratch;   log [log_steps,B,3] float64 ring of (E_pot, E_kin, edges found) per step and graph;
 *   state [4] int64 = (step, halt code, step at which it halted, mode).
 *
 * hermnet_md_advance   halt code != 0: nothing.  mode 1 ("prime"): pos32 = float(x), nothing else.  Otherwise x0, v0, image0
 *   = x, v, image, then NVE (velocity Verlet) v += kick f_prev, x += dt v, or with HN_MD_LANGEVIN BAOAB: v += kick f_prev,
 *   x += dt/2 v, v = c1 v + sigma xi, x += dt/2 v; with HN_MD_WRAP s = x cell^-1, x -= floor(s) cell, image += floor(s);
 *   pos32 = float(x).
 * hermnet_md_finish    halt code != 0: nothing.  The step's code = the list's flags total[1] (low 8 bits; bit 2 also where
 *   total[0] > capacity) | HN_MD_HALT_NONFINITE if an energy [B] is not finite.  mode 1: f_prev = forces if the code is 0;
 *   mode = 0 (no kick, no log row, no step).  Code != 0: x, v, image = x0, v0, image0, pos32 = float(x), state = (step, code,
 *   step, 0), no log row: the state is that of the last completed step and every later replay changes nothing.  Code 0:
 *   v += kick forces, f_prev = forces, log[step % log_steps][g] = (energy[g], sum of half_mass |v|^2 over graph g -- float64,
 *   fixed order, no atomics --, total[0]), step += 1.  Three launches; only the last one writes `state`.
 * Noise: xi of (seed, step, atom) from Philox4x32-10 with key (seed low, seed high) and counters (atom, step low, step high,
 *   stream): stream 0 gives words w0..w3, stream 1 w4..w7; u(a, b) = ((a >> 5) 2^26 + (b >> 6)); Box-Muller in float64:
 *   r = sqrt(-2 log((u(w0,w1) + 1) 2^-53)), t = 2 pi u(w2,w3) 2^-53, xi = (r cos t, r sin t, the cosine branch of w4..w7).
 *   It depends on nothing else (launch geometry, how a run is split).  hermnet_md_noise writes out_words [n,8] uint32 and
 *   out_gauss [n,3] float64 (either may be NULL) for atoms 0..n-1.
 * The per-atom arithmetic is IEEE +, x, floor on doubles, one rounding each, no contraction; the hermnet_host_md_* twins run
 * the same text in a CPU loop on HOST pointers (no stream), bit for bit what the device computes for the same forces and xi. */
#define HN_MD_LANGEVIN 1
#define HN_MD_WRAP 2
#define HN_MD_HALT_NONFINITE 256
int hermnet_md_advance(int num_atoms, int num_graphs, int flags, double dt, unsigned long seed, double* x, double* v, double* x0,
                       double* v0, int* image, int* image0, const float* f_prev, const double* kick, const double* c1,
                       const double* sigma, const long* batch, const float* cell, const double* inv_cell, float* pos32,
                       const long* state, void* stream);
int hermnet_md_finish(int num_atoms, int num_graphs, const int* graph_ptr, const float* forces, const float* energy,
                      const long* total, long capacity, double* x, double* v, const double* x0, const double* v0, int* image,
                      const int* image0, float* f_prev, const double* kick, const double* half_mass, float* pos32,
                      double* ke_atom, double* log, long log_steps, long* state, void* stream);
int hermnet_md_noise(unsigned long seed, unsigned long step, int n, unsigned* out_words, double* out_gauss, void* stream);
int hermnet_host_md_advance(int num_atoms, int num_graphs, int flags, double dt, unsigned long seed, double* x_host,
                            double* v_host, double* x0_host, double* v0_host, int* image_host, int* image0_host,
                            const float* f_prev_host, const double* kick_host, const double* c1_host, const double* sigma_host,
                            const long* batch_host, const float* cell_host, const double* inv_cell_host, float* pos32_host,
                            const long* state_host);
int hermnet_host_md_finish(int num_atoms, int num_graphs, const int* graph_ptr_host, const float* forces_host,
                           const float* energy_host, const long* total_host, long capacity, double* x_host, double* v_host,
                           const double* x0_host, const double* v0_host, int* image_host, const int* image0_host,
                           float* f_prev_host, const double* kick_host, const double* half_mass_host, float* pos32_host,
                           double* ke_atom_host, double* log_host, long log_steps, long* state_host);
int hermnet_host_md_noise(unsigned long seed, unsigned long step, int n, unsigned* out_words_host, double* out_gauss_host);

/* Device-resident NPT: a Berendsen barostat inside the replayed MD step (added within ABI v13: new entry points only;
 * hermnet_amd/md.py: DeviceNPT; csrc/md_kernels.hip, npt_step.h).  hermnet_md_finish_npt takes the place of hermnet_md_finish
 * behind the force backward of a step captured WITH the virial kernels and with the cell as a device-side input; the advance
 * is hermnet_md_advance.  One force evaluation per step; the scaling ends a committed step (as GROMACS orders it) and is
 * ASE's NPTBerendsen formula.  Units: eV, Angstrom, fs; pressures in eV / A^3.
 *
 * Caller-owned state beside hermnet_md_finish's:   virial [B,9] float32 the step's virial output (stress = -sym(W) / V);
 *   cell64 [B,9] float64 the cell -- the truth --, cell32 [B,9] float32 its rounding: the tensor search, edge geometry and
 *   virial kernels read, inv_cell [B,9] float64 the inverse of the WIDENED cell32 (adjugate over determinant), the one
 *   hermnet_md_advance wraps with;   mu [B,9] float64 the last scaling matrix;   clamped [B] int64 how often the safety
 *   conditions acted;   pressure [B] the targets P0, coupling_c [B] = (dt / taup) compressibility / 3;   batch [N] int64 or
 *   NULL (one graph);   log [log_steps,B,5] = (E_pot, E_kin, edges found, pressure, volume).
 *
 * hermnet_md_finish_npt   halt code != 0: nothing.  Mode 1, and a step whose code is not 0: as hermnet_md_finish -- cell64,
 *   cell32, inv_cell, mu are NOT touched (a void step restores x, v, image alone: the cell needs no backup because only
 *   committed steps scale).  Code 0: v += kick forces, f_prev = forces; then per graph g:
 *     K_ab = sum m_i v_ia v_ib over xx, yy, zz, xy, xz, yz (m = 2 half_mass; a term is (m v_a) v_b), six sums in the
 *       canonical order of hermnet_relax_finish;  E_kin = ((K_xx + K_yy) + K_zz) / 2;
 *     V = |det cell64|, det = (c0 (c4 c8 - c5 c7) + c1 (c5 c6 - c3 c8)) + c2 (c3 c7 - c4 c6);
 *     P_ab = (K_ab + (W_ab + W_ba) / 2) / V with W widened to float64;  P = ((P_xx + P_yy) + P_zz) / 3;
 *     e_ab: HN_MD_BARO_ISOTROPIC c (P0 - P) on the diagonal;  HN_MD_BARO_AXES c (P0 - P_kk) on the diagonal entries k with
 *       bit k of `mask` set, 0 elsewhere;  HN_MD_BARO_FULL c (P0 delta_ab - P_ab);  every e_ab is clamped to +-max_strain;
 *       an entry of P that is not finite: e = 0 (these two are safety conditions: a scaled cell cannot be taken back);
 *     mu = I - e;  cell64 <- cell64 mu (rows are lattice vectors; an entry is (c_i0 mu_0j + c_i1 mu_1j) + c_i2 mu_2j);
 *     cell32 = float(cell64);  inv_cell = adj(double(cell32)) / det(double(cell32));  clamped += 1 where a condition acted;
 *     log[step % log_steps][g] = (energy[g], E_kin, total[0], P, V) -- the pressure mu was made from, the volume before it;
 *   then every atom (held ones too) x <- x mu of its graph, pos32 = float(x); images and velocities stay;  step += 1.
 *   Four launches: hermnet_md_finish's per-atom kernel, one 256-lane workgroup per graph, the per-atom scaling, and the
 *   single workgroup that alone writes `state`.
 * hermnet_host_md_finish_npt runs the same text on HOST pointers (no stream), the sums in the canonical order: bit for bit
 *   what the device computes for the same forces and virial.
 * HN_ERR_BAD_ARG: hermnet_md_finish's, a NULL virial / pressure / coupling_c / cell64 / cell32 / inv_cell / mu / clamped,
 *   an unknown coupling, mask bits above 7, max_strain <= 0 (or NaN). */
#define HN_MD_BARO_ISOTROPIC 0
#define HN_MD_BARO_AXES 1
#define HN_MD_BARO_FULL 2
int hermnet_md_finish_npt(int num_atoms, int num_graphs, const int* graph_ptr, const long* batch, const float* forces,
                          const float* energy, const float* virial, const long* total, long capacity, int coupling, int mask,
                          double max_strain, const double* pressure, const double* coupling_c, double* x, double* v,
                          const double* x0, const double* v0, int* image, const int* image0, float* f_prev, const double* kick,
                          const double* half_mass, float* pos32, double* ke_atom, double* cell64, float* cell32,
                          double* inv_cell, double* mu, long* clamped, double* log, long log_steps, long* state, void* stream);
int hermnet_host_md_finish_npt(int num_atoms, int num_graphs, const int* graph_ptr_host, const long* batch_host,
                               const float* forces_host, const float* energy_host, const float* virial_host,
                               const long* total_host, long capacity, int coupling, int mask, double max_strain,
                               const double* pressure_host, const double* coupling_c_host, double* x_host, double* v_host,
                               const double* x0_host, const double* v0_host, int* image_host, const int* image0_host,
                               float* f_prev_host, const double* kick_host, const double* half_mass_host, float* pos32_host,
                               double* ke_atom_host, double* cell64_host, float* cell32_host, double* inv_cell_host,
                               double* mu_host, long* clamped_host, double* log_host, long log_steps, long* state_host);

/* Device-resident FIRE relaxation of a batch of structures (added within ABI v13: new entry points only;
 * hermnet_amd/relax.py: DeviceRelax; csrc/relax_kernels.hip, relax_driver.h, relax_step.h).  As for hermnet_md_*:
 * hermnet_relax_advance is enqueued in FRONT of the captured neighbour search and hermnet_relax_finish BEHIND the force
 * backward, so that one replay of the step's hipGraph is one force evaluation of the optimiser.  The optimiser is ASE's
 * FIRE (dt, dtmax, maxstep, fmax are arguments; Nmin 5, finc 1.1, fdec 0.5, astart 0.1, fa 0.99), applied to every graph on
 * its own: a graph whose largest force is below its threshold freezes while the others keep going.  Units: eV, Angstrom;
 * FIRE's time is a parameter.
 *
 * Caller-owned state (all allocated outside the capture):
 *   x, x0 [N,3] float64 coordinates and their start-of-step backup;   v [N,3] float64 FIRE's velocities;   image, image0
 *   [N,3] int32 as for hermnet_md_*;   f_prev [N,3] float32 the forces of a graph's last evaluation while it was moving;
 *   fixed [N] uint8 or NULL: an atom that is held counts as f = 0 everywhere, keeps v = 0 and is never moved;   batch,
 *   graph_ptr, cell, inv_cell, pos32 as for hermnet_md_*;   fmax_graph [B] float64 or NULL (then `fmax` for all);
 *   gf [B,5] float64 = (dt, a, scale, fnorm, energy) and gi [B,4] int64 = (nsteps, fresh, converged, conv_step) per graph --
 *   scale is what the next advance multiplies v with; a run starts from scale 0, fresh 1, converged 0, v 0 --, gf_new / gi_new
 *   their scratch copies;   log [log_steps,B,4] float64 ring of (E_pot, max |f_i|, dt, edges found) per evaluation and graph;
 *   state [4] int64 = (step, halt code, step at which it halted, done).
 *
 * hermnet_relax_advance   halt code != 0: nothing.  For every atom of a graph that has not converged: x0, image0 = x, image,
 *   and unless it is held x += scale_g v, then with HN_MD_WRAP (the only flag) the wrap of hermnet_md_advance.  All atoms:
 *   pos32 = float(x).  scale starts at 0: the first replay evaluates the start coordinates.
 * hermnet_relax_finish    halt code != 0 or done: nothing.  The step's code is hermnet_md_finish's.  Code != 0: the step is
 *   void -- x, image = x0, image0 and pos32 = float(x) for the graphs that moved, v and the per-graph state untouched, state
 *   = (step, code, step, 0), no log row.  Code 0, per graph that has not converged, with f = float64(forces) (0 where held):
 *   P = sum f.v, ff = sum f.f, vv = sum v.v, fm2 = max |f_i|^2;  fm2 < fmax^2 (an empty graph too): converged, conv_step =
 *   step, scale = 0, v = 0.  Otherwise: fresh: dt = `dt`, a = astart, nsteps = 0, fresh = 0;  else P > 0: v = (1 - a) v +
 *   (ff > 0 ? (a / sqrt(ff)) sqrt(vv) : 0) f, then if nsteps > Nmin dt = min(dt finc, dtmax), a = a fa, then nsteps += 1;
 *   else v = 0, a = astart, dt = dt fdec, nsteps = 0.  Then v += dt f;  s = sum v.v;  nd = dt sqrt(s);  scale = nd > maxstep ?
 *   dt (maxstep / nd) : dt;  f_prev = forces;  fnorm = sqrt(fm2), energy = energy[g].  Every graph: log[step % log_steps][g]
 *   = (energy, fnorm, dt, total[0]).  step += 1; done = 1 once every graph has converged.
 *   Two launches: one 256-lane workgroup per graph, then one workgroup that alone writes state, gf and gi (from gf_new /
 *   gi_new), so every workgroup of a step reads the state the step began with.
 * A per-graph sum takes ONE order: lane l of 256 adds the terms of atoms lo+l, lo+l+256, ... ascending from 0.0, the
 *   partials are folded part[l] += part[l+m], m = 128 ... 1; an atom's term is (t0 + t1) + t2; no atomics.  `/` and sqrt
 *   appear in the per-graph scalars alone.  The hermnet_host_relax_* twins run the same text, in this order, on HOST
 *   pointers (no stream): bit for bit what the device computes for the same forces.
 * HN_ERR_BAD_ARG: a NULL state / gf / gi (or any array with num_atoms > 0), num_graphs < 1, log_steps < 1, a flag other
 *   than HN_MD_WRAP, dt, dtmax, maxstep or fmax not positive.  num_atoms = 0 is served. */
int hermnet_relax_advance(int num_atoms, int num_graphs, int flags, double* x, double* x0, const double* v, int* image, int* image0,
                          const unsigned char* fixed, const long* batch, const float* cell, const double* inv_cell, float* pos32,
                          const long* state, const double* gf, const long* gi, void* stream);
int hermnet_relax_finish(int num_atoms, int num_graphs, const int* graph_ptr, const float* forces, const float* energy,
                         const long* total, long capacity, double dt, double dtmax, double maxstep, double fmax,
                         const double* fmax_graph, double* x, double* v, const double* x0, int* image, const int* image0,
                         float* f_prev, const unsigned char* fixed, float* pos32, double* gf, long* gi, double* gf_new,
                         long* gi_new, double* log, long log_steps, long* state, void* stream);
int hermnet_host_relax_advance(int num_atoms, int num_graphs, int flags, double* x_host, double* x0_host, const double* v_host,
                               int* image_host, int* image0_host, const unsigned char* fixed_host, const long* batch_host,
                               const float* cell_host, const double* inv_cell_host, float* pos32_host, const long* state_host,
                               const double* gf_host, const long* gi_host);
int hermnet_host_relax_finish(int num_atoms, int num_graphs, const int* graph_ptr_host, const float* forces_host,
                              const float* energy_host, const long* total_host, long capacity, double dt, double dtmax,
                              double maxstep, double fmax, const double* fmax_graph_host, double* x_host, double* v_host,
                              const double* x0_host, int* image_host, const int* image0_host, float* f_prev_host,
                              const unsigned char* fixed_host, float* pos32_host, double* gf_host, long* gi_host,
                              double* gf_new_host, long* gi_new_host, double* log_host, long log_steps, long* state_host);

/* Device-resident CELL relaxation: FIRE on atoms and cell together (added within ABI v13: new entry points only;
 * hermnet_amd/relax.py: DeviceCellRelax; csrc/cellrelax_kernels.hip, relax_driver.h, cellrelax_step.h).  The model is ASE's
 * UnitCellFilter under ASE's FIRE, every graph on its own.  hermnet_cellrelax_advance is enqueued in FRONT of the neighbour search of a step
 * captured WITH the virial kernels and with the cell as a device-side input, hermnet_cellrelax_finish BEHIND the force
 * backward: one replay is one force-and-stress evaluation.  Units: eV, Angstrom; pressures in eV / A^3.
 *
 * Per graph, C0 = cell0 (float64, constant) and cf = cell_factor:  F (deform) starts as I, C = C0 F^T (cell64);  the
 *   generalised coordinates are q_i = x_i F^-T (the state; x is derived) and the rows G = cf F (rows);  the generalised forces
 *   fq_i = f_i F (0 where held) and fG = proj(S F^-T) / cf, S = sym(W) - p V I, W = float64(virial), V = |det C|, p =
 *   pressure[g];  proj in this order: HN_CELLRELAX_HYDROSTATIC replaces by (tr / 3) I, then x mask [9] entry-wise, then
 *   HN_CELLRELAX_CONSTANT_VOLUME subtracts tr / 3 from the diagonal.  The objective is the enthalpy E + p V.
 * Caller-owned state beside hermnet_relax_*'s (x0, image0, f_prev, fixed, batch, graph_ptr, fmax_graph, gf, gi, gf_new,
 *   gi_new, state as there; v [N,3] the velocities of q):   q, q0 [N,3] float64 and x [N,3] = q F^T;   cell0, inv_cell0 [B,9]
 *   float64 (the inverse by adjugate over determinant), cell_factor [B] > 0;   rows, rows0, rows_v [B,9] G, its start-of-step
 *   backup and its velocities;   deform, deform_inv, cell64 [B,9], det_f [B] (det F of the last advance; 1 at the start);
 *   cell32 [B,9] float32 = float(C): the tensor search, edge geometry and virial kernels read;   obs [B,11] = (V, tr W / 3V,
 *   stress [9] = -sym(W) / V) of a graph's last evaluation while it moved;   mask_host [9]: a HOST array, read at the call;
 *   log [log_steps,B,6] = (enthalpy, max generalised force, dt, edges found, V, tr W / 3V);   gf's energy is the enthalpy,
 *   its fnorm the largest generalised force.
 *
 * hermnet_cellrelax_advance   halt code != 0: nothing.  First kernel, per graph that has not converged: rows0 = rows, rows +=
 *   scale rows_v, F = rows / cf, C_ij = (C0_i0 F_j0 + C0_i1 F_j1) + C0_i2 F_j2, cell32 = float(C), det_f = det F, F^-1 =
 *   adj(F) / det F.  Second kernel, per atom of such a graph: q0, x0, image0 = q, x, image; unless held q += scale v, then with
 *   HN_MD_WRAP (the only flag) the wrap of hermnet_md_advance on q against cell0 / inv_cell0;  x_j = (q_0 F_j0 + q_1 F_j1) +
 *   q_2 F_j2.  All atoms: pos32 = float(x).  A converged graph is not written, its cell included.
 * hermnet_cellrelax_finish    halt code != 0 or done: nothing.  The step's code is hermnet_md_finish's, with
 *   HN_MD_HALT_NONFINITE also for a virial entry that is not finite or a det_f that is not > 0.  Code != 0: void -- for the
 *   graphs that moved q, x, image = q0, x0, image0, pos32 = float(x), rows = rows0 and deform, deform_inv, cell64, cell32 made
 *   of it again; velocities, rows_v and the per-graph state untouched; state = (step, code, step, 0); no log row.  Code 0:
 *   hermnet_relax_finish's text on the n + 3 rows (fq_i, vq_i; fG_r, rows_v_r): P, ff, vv and the clamp's s are the atoms'
 *   canonical sums, THEN the three cell rows' terms added in row order 0, 1, 2; fm2 is the maximum over atoms and rows.
 *   Launches: one 256-lane workgroup per graph, then the workgroup that alone writes state, gf and gi.
 * The hermnet_host_cellrelax_* twins run the same text on HOST pointers (no stream), bit for bit.
 * HN_ERR_BAD_ARG: hermnet_relax_*'s, a NULL cell array / virial / pressure / obs / mask_host, a mask entry that is not finite,
 *   unknown flag bits; the host twins also refuse cell_factor <= 0 (the device entry points cannot read it). */
#define HN_CELLRELAX_HYDROSTATIC 1
#define HN_CELLRELAX_CONSTANT_VOLUME 2
int hermnet_cellrelax_advance(int num_atoms, int num_graphs, int flags, double* q, double* q0, double* x, double* x0,
                              const double* v, int* image, int* image0, const unsigned char* fixed, const long* batch,
                              const double* cell0, const double* inv_cell0, const double* cell_factor, double* rows, double* rows0,
                              const double* rows_v, double* deform, double* deform_inv, double* det_f, double* cell64,
                              float* cell32, float* pos32, const long* state, const double* gf, const long* gi, void* stream);
int hermnet_cellrelax_finish(int num_atoms, int num_graphs, int flags, const int* graph_ptr, const float* forces,
                             const float* energy, const float* virial, const long* total, long capacity, double dt, double dtmax,
                             double maxstep, double fmax, const double* fmax_graph, const double* pressure,
                             const double* mask_host, const double* cell0, const double* inv_cell0, const double* cell_factor,
                             double* q, const double* q0, double* x, const double* x0, double* v, int* image, const int* image0,
                             float* f_prev, const unsigned char* fixed, float* pos32, double* rows, const double* rows0,
                             double* rows_v, double* deform, double* deform_inv, double* det_f, double* cell64, float* cell32,
                             double* obs, double* gf, long* gi, double* gf_new, long* gi_new, double* log, long log_steps,
                             long* state, void* stream);
int hermnet_host_cellrelax_advance(int num_atoms, int num_graphs, int flags, double* q_host, double* q0_host, double* x_host,
                                   double* x0_host, const double* v_host, int* image_host, int* image0_host,
                                   const unsigned char* fixed_host, const long* batch_host, const double* cell0_host,
                                   const double* inv_cell0_host, const double* cell_factor_host, double* rows_host,
                                   double* rows0_host, const double* rows_v_host, double* deform_host, double* deform_inv_host,
                                   double* det_f_host, double* cell64_host, float* cell32_host, float* pos32_host,
                                   const long* state_host, const double* gf_host, const long* gi_host);
int hermnet_host_cellrelax_finish(int num_atoms, int num_graphs, int flags, const int* graph_ptr_host, const float* forces_host,
                                  const float* energy_host, const float* virial_host, const long* total_host, long capacity,
                                  double dt, double dtmax, double maxstep, double fmax, const double* fmax_graph_host,
                                  const double* pressure_host, const double* mask_host, const double* cell0_host,
                                  const double* inv_cell0_host, const double* cell_factor_host, double* q_host,
                                  const double* q0_host, double* x_host, const double* x0_host, double* v_host, int* image_host,
                                  const int* image0_host, float* f_prev_host, const unsigned char* fixed_host, float* pos32_host,
                                  double* rows_host, const double* rows0_host, double* rows_v_host, double* deform_host,
                                  double* deform_inv_host, double* det_f_host, double* cell64_host, float* cell32_host,
                                  double* obs_host, double* gf_host, long* gi_host, double* gf_new_host, long* gi_new_host,
                                  double* log_host, long log_steps, long* state_host);

/* Device-resident nudged elastic band: climbing-image NEB with improved tangents under FIRE on the whole band (added within
 * ABI v13: new entry points only; hermnet_amd/neb.py: DeviceNEB; csrc/neb_kernels.hip, neb_step.h).  The captured step is
 * bracketed by hermnet_relax_advance -- unchanged, WITHOUT HN_MD_WRAP, so displacements between images are plain differences
 * -- and hermnet_neb_finish behind the force backward: one replay is one force evaluation of every image.
 *
 * The B graphs are the images; band_ptr [K+1] int32 splits them into K bands of >= 3 images of one atom count, band_of [B]
 * int32 names each image's band.  A band's first and last image are end points: evaluated, never moved -- their gf / gi rows
 * are converged = 1, scale = 0 from the start and are never written.  Caller-owned state as for hermnet_relax_* (x, x0, v,
 * image, image0, f_prev, fixed, pos32, graph_ptr, log [log_steps,B,4], state), and: gf [B,5] / gi [B,4] hermnet_relax_*'s rows
 * per image -- an interior image's row is its band's FIRE state (dt, a, scale, max |g_a| over the band; nsteps, fresh,
 * converged, conv_step) with the image's own energy --, k_band, fmax_band [K] float64 (spring constant eV/A^2, threshold
 * eV/A), obs [B,4] = (energy, max |g_a|, |t2|, ft) per image (end points: the energy, 0, 0, 0), climber [K] int64 the
 * climbing image's index within its band (-1: none);  scratch: g [N,3], isum [B,4], csum [B], bf_new [K,5], bi_new [K,4],
 * climber_new [K].
 *
 * hermnet_neb_finish    halt code != 0 or done: nothing.  The step's code is hermnet_md_finish's.  Code != 0: void -- x, image
 *   = x0, image0 and pos32 = float(x) for the interior images of the bands that moved; velocities and all state untouched;
 *   state = (step, code, step, 0); no log row.  Code 0, per band that has not converged, per interior image i with energies
 *   Em, E0, Ep = float64(energy[i-1], [i], [i+1]), F = float64(forces) (0 where held), t1 = x_i - x_(i-1), t2 = x_(i+1) - x_i
 *   (0 where held):  (c1, c2) = (0, 1) if Ep > E0 > Em;  (1, 0) if Ep < E0 < Em;  else with hi / lo = max / min(|Ep - E0|,
 *   |Em - E0|): (lo, hi) if Ep > Em else (hi, lo);  T = c2 t2 + c1 t1;  canonical sums over the image's atoms t1.t1, t2.t2,
 *   T.T, F.T;  inv = T.T == 0 ? 0 : 1 / sqrt(T.T);  ft = (F.T) inv;  spring = k (sqrt(t2.t2) - sqrt(t1.t1));  par = spring - ft,
 *   or -2 ft on the climbing image (climb = 1: the band's interior image of largest energy, ties to the lowest index);  g_a =
 *   F_a + par (T_a inv);  canonical sums g.v, g.g, v.v, max |g_a|^2 per image, folded over the band's interior images in
 *   ascending order from 0.0;  then hermnet_relax_finish's FIRE on those sums with g for f, the clamp's sum v.v per image and
 *   then over the images in the same order;  f_prev = forces.  A band whose max |g_a| < fmax_band[k] converges: conv_step =
 *   step, scale = 0, v = 0, and it is never written again.  Every image: log[step % log_steps][i] = (obs energy, obs max |g_a|,
 *   the band's dt, total[0]).  step += 1; done = 1 once every band has converged.
 *   Three launches: one 256-lane workgroup per image (tangent, scalars, g, partials), one per image (the band's sums, FIRE,
 *   velocities, the clamp's partial), then the one workgroup that alone writes state, gf, gi and climber.  No atomics; no
 *   workgroup reads what another of the same launch writes.
 * hermnet_host_neb_finish runs the same text on HOST pointers (no stream), bit for bit.
 * HN_ERR_BAD_ARG: a NULL pointer (fixed may be NULL; the per-atom arrays with num_atoms > 0), num_graphs < 3, num_bands < 1
 *   or > num_graphs / 3, log_steps < 1, capacity < 0, climb not 0 or 1, dt, dtmax or maxstep not positive; the host twin also
 *   refuses bands that do not tile the graphs, a band shorter than 3, images of unequal atom count, a band_of that disagrees,
 *   k < 0 and fmax <= 0 (the device entry point cannot read them). */
int hermnet_neb_finish(int num_atoms, int num_graphs, int num_bands, int climb, const int* graph_ptr, const int* band_ptr,
                       const int* band_of, const float* forces, const float* energy, const long* total, long capacity, double dt,
                       double dtmax, double maxstep, const double* k_band, const double* fmax_band, double* x, double* v,
                       const double* x0, int* image, const int* image0, float* f_prev, const unsigned char* fixed, float* pos32,
                       double* gf, long* gi, double* obs, long* climber, double* g, double* isum, double* csum, double* bf_new,
                       long* bi_new, long* climber_new, double* log, long log_steps, long* state, void* stream);
int hermnet_host_neb_finish(int num_atoms, int num_graphs, int num_bands, int climb, const int* graph_ptr_host,
                            const int* band_ptr_host, const int* band_of_host, const float* forces_host, const float* energy_host,
                            const long* total_host, long capacity, double dt, double dtmax, double maxstep,
                            const double* k_band_host, const double* fmax_band_host, double* x_host, double* v_host,
                            const double* x0_host, int* image_host, const int* image0_host, float* f_prev_host,
                            const unsigned char* fixed_host, float* pos32_host, double* gf_host, long* gi_host, double* obs_host,
                            long* climber_host, double* g_host, double* isum_host, double* csum_host, double* bf_new_host,
                            long* bi_new_host, long* climber_new_host, double* log_host, long log_steps, long* state_host);

/* Device-resident temperature replica exchange (added within ABI v13: new entry points only; hermnet_amd/remd.py: DeviceREMD;
 * csrc/remd_kernels.hip, remd_step.h).  The captured step is a Langevin step of B replicas of ONE system: hermnet_md_advance,
 * unchanged, in front of the search, and hermnet_remd_finish in the place of hermnet_md_finish behind the force backward.
 *
 * One ladder of R = B rungs.  Caller-owned state beside hermnet_md_finish's (log is [log_steps,B,5] here):  beta [R] float64
 * = 1 / (kB T_r);  up, down [R-1] float64 = sqrt(T_(r+1) / T_r), sqrt(T_r / T_(r+1));  sigma_table [R, N/B] float64, row r
 * = hermnet_md_advance's sigma of one replica at T_r;  sigma [N] float64, the array hermnet_md_advance reads;  rung [B] int64
 * the rung replica g holds and replica_at [R] int64 its inverse (both start as the identity: replicas stay where they are
 * in the batch, temperatures travel);  attempts, accepts [R-1] int64 counters per pair (r, r+1);  scratch: rung_new [B] int64,
 * vscale [B] float64, outcome [R-1] int64 (0 not tried, 1 rejected, 2 accepted).  `seed` is hermnet_md_advance's.
 *
 * hermnet_remd_finish    halt code != 0: nothing.  Mode 1, and a step whose code is not 0: as hermnet_md_finish -- rung,
 *   replica_at, sigma and the counters untouched, no attempt.  Code 0: hermnet_md_finish's second kick, f_prev and ke_atom;
 *   then, where (step + 1) % exchange_interval == 0, attempt a = (step + 1) / exchange_interval - 1 tries the pairs (r, r+1)
 *   with r % 2 == a % 2, r + 1 < R:  with ga = replica_at[r], gb = replica_at[r+1],  delta = (beta[r] - beta[r+1]) *
 *   ((double)energy[ga] - (double)energy[gb]);  accepted iff delta >= 0 or log(u) < delta,  u = (u(w0,w1) + 1) 2^-53 with
 *   hermnet_md_advance's u(,) and w = Philox4x32-10 of key (seed low, seed high), counter (r, step low, step high, 2) --
 *   streams 0 and 1 are the atoms' noise.  An accepted pair swaps rungs; every velocity of ga is multiplied by up[r], of gb by
 *   down[r]; sigma[i] = sigma_table[new rung][i - first atom of the replica];  attempts[r] counts tried, accepts[r] accepted
 *   pairs.  log[step % log_steps][g] = (energy[g], the canonical sum of ke_atom over replica g -- taken before any rescaling
 *   --, total[0], rung[g] during the step, rung[g] behind the step's exchange);  step += 1.
 *   Four launches: hermnet_md_finish's per-atom kernel; one workgroup with a lane per pair that writes the scratch alone; one
 *   256-lane workgroup per replica (E_kin, the log row, v and sigma where its rung changed); and the one workgroup that alone
 *   writes rung, replica_at, the counters and state.  No atomics; no workgroup reads what another of the same launch writes.
 * hermnet_host_remd_finish runs the same text on HOST pointers (no stream), bit for bit but for the last digits of log(u).
 * HN_ERR_BAD_ARG: hermnet_md_finish's, a NULL pointer, num_graphs < 2, num_atoms no multiple of num_graphs,
 *   exchange_interval < 1; the host twin also refuses replicas that do not tile the atoms in equal ranges and a rung /
 *   replica_at that is no permutation with its inverse (the device entry point cannot read them). */
int hermnet_remd_finish(int num_atoms, int num_graphs, const int* graph_ptr, const float* forces, const float* energy,
                        const long* total, long capacity, long exchange_interval, unsigned long seed, double* x, double* v,
                        const double* x0, const double* v0, int* image, const int* image0, float* f_prev, const double* kick,
                        const double* half_mass, float* pos32, double* ke_atom, const double* beta, const double* up,
                        const double* down, const double* sigma_table, double* sigma, long* rung, long* replica_at,
                        long* rung_new, double* vscale, long* outcome, long* attempts, long* accepts, double* log,
                        long log_steps, long* state, void* stream);
int hermnet_host_remd_finish(int num_atoms, int num_graphs, const int* graph_ptr_host, const float* forces_host,
                             const float* energy_host, const long* total_host, long capacity, long exchange_interval,
                             unsigned long seed, double* x_host, double* v_host, const double* x0_host, const double* v0_host,
                             int* image_host, const int* image0_host, float* f_prev_host, const double* kick_host,
                             const double* half_mass_host, float* pos32_host, double* ke_atom_host, const double* beta_host,
                             const double* up_host, const double* down_host, const double* sigma_table_host,
                             double* sigma_host, long* rung_host, long* replica_at_host, long* rung_new_host,
                             double* vscale_host, long* outcome_host, long* attempts_host, long* accepts_host, double* log_host,
                             long log_steps, long* state_host);

/* Device-resident ring-polymer path-integral MD (added within ABI v13: new entry points only; hermnet_amd/pimd.py: DevicePIMD;
 * csrc/pimd_kernels.hip, pimd_step.h).  The captured step is one BAOAB step of a ring polymer whose P = B beads are the graphs
 * of the batch, all ONE system of n_rep = N / B atoms (atom a of bead j is row j n_rep + a): hermnet_pimd_advance in the place
 * of hermnet_md_advance in front of the search, hermnet_pimd_finish in the place of hermnet_md_finish behind the force
 * backward.  Convention: Ceriotti et al., J. Chem. Phys. 133, 124104 (2010) -- every bead feels the full potential, the
 * extended system is sampled at P T, omega_P = P kB T / hbar, omega_k = 2 omega_P sin(k pi / P).
 *
 * Caller-owned state beside hermnet_md_advance's / _finish's (log is [log_steps,B,5] here), every table made on the host in
 * float64:  cmat [P,P] the real orthogonal normal-mode matrix C[j][k] at j P + k (k = 0: sqrt(1/P); 0 < 2k < P: sqrt(2/P)
 * cos(2 pi j k / P); 2k = P: sqrt(1/P) (-1)^j; 2k > P: sqrt(2/P) sin(2 pi j k / P));  cs, sw, ws [P] = cos(omega_k t),
 * sin(omega_k t) / omega_k (t for k = 0), omega_k sin(omega_k t), with t = dt / 2 under HN_MD_LANGEVIN and t = dt without;
 * c1 [P] = exp(-dt gamma_k) and sigma [P, n_rep] = sqrt(kB P T (1 - c1_k^2) / m_a) (both read under HN_MD_LANGEVIN alone);
 * inv_beads = 1 / P;  spring_c [n_rep] = m_a omega_P^2 / 2 (0 for an atom that is held);  centroid [n_rep,3] float64 scratch.
 *
 * hermnet_pimd_advance   halt code != 0: nothing.  mode 1: pos32 = float(x), nothing else.  Otherwise x0, v0, image0 = x, v,
 *   image, then per atom whose kick is not 0:  v_j += kick f_prev_j on every bead;  per component q~_k = sum_j C[j][k] q_j and
 *   v~_k likewise (from 0.0, ascending j);  the free flight q~' = cs_k q~ + sw_k v~, v~' = cs_k v~ - ws_k q~ (the old q~);
 *   under HN_MD_LANGEVIN v~ = c1_k v~ + sigma[k][a] xi with hermnet_md_advance's xi of (seed, step, k n_rep + a), and the
 *   free flight again;  q_j = sum_k C[j][k] q~_k (from 0.0, ascending k), v likewise;  with HN_MD_WRAP the centroid
 *   c = (ascending sum of the q_j) inv_beads takes hermnet_md_advance's wrap against cell / inv_cell of graph 0, and EVERY
 *   bead of the atom loses the same floor(s) cell and gains the same floor(s) in its image.  An atom whose kick is 0 (an
 *   infinite mass) keeps x, v and image.  All atoms: pos32 = float(x); centroid[a] = c (wrapped where the atom was).
 *   One launch: a 256-lane workgroup per tile of 256 / P atoms x P lanes, the transform through LDS; no atomics.
 * hermnet_pimd_finish    hermnet_md_finish, but for the log row:  log[step % log_steps][j] = (energy[j], E_kin_j, total[0],
 *   spring_j = sum_a spring_c[a] |x_(j,a) - x_(j+1,a)|^2 (cyclic in j), vir_j = sum_a (x_(j,a) - centroid[a]) . forces_(j,a)),
 *   the three sums over the atoms that are not held, float64 in hermnet_md_finish's fixed order.  Three launches.
 * The hermnet_host_pimd_* twins run the same text on HOST pointers (no stream), bit for bit what the device computes for the
 * same forces and xi.  HN_ERR_BAD_ARG: hermnet_md_advance's / _finish's, a NULL table, num_graphs > 128, num_atoms no multiple
 * of num_graphs; the host finish also refuses beads that do not tile the atoms in equal ranges. */
int hermnet_pimd_advance(int num_atoms, int num_graphs, int flags, unsigned long seed, double inv_beads, double* x, double* v,
                         double* x0, double* v0, int* image, int* image0, const float* f_prev, const double* kick,
                         const double* cmat, const double* cs, const double* sw, const double* ws, const double* c1,
                         const double* sigma, const float* cell, const double* inv_cell, float* pos32, double* centroid,
                         const long* state, void* stream);
int hermnet_pimd_finish(int num_atoms, int num_graphs, const int* graph_ptr, const float* forces, const float* energy,
                        const long* total, long capacity, double* x, double* v, const double* x0, const double* v0, int* image,
                        const int* image0, float* f_prev, const double* kick, const double* half_mass, float* pos32,
                        double* ke_atom, const double* spring_c, const double* centroid, double* log, long log_steps,
                        long* state, void* stream);
int hermnet_host_pimd_advance(int num_atoms, int num_graphs, int flags, unsigned long seed, double inv_beads, double* x_host,
                              double* v_host, double* x0_host, double* v0_host, int* image_host, int* image0_host,
                              const float* f_prev_host, const double* kick_host, const double* cmat_host, const double* cs_host,
                              const double* sw_host, const double* ws_host, const double* c1_host, const double* sigma_host,
                              const float* cell_host, const double* inv_cell_host, float* pos32_host, double* centroid_host,
                              const long* state_host);
int hermnet_host_pimd_finish(int num_atoms, int num_graphs, const int* graph_ptr_host, const float* forces_host,
                             const float* energy_host, const long* total_host, long capacity, double* x_host, double* v_host,
                             const double* x0_host, const double* v0_host, int* image_host, const int* image0_host,
                             float* f_prev_host, const double* kick_host, const double* half_mass_host, float* pos32_host,
                             double* ke_atom_host, const double* spring_c_host, const double* centroid_host, double* log_host,
                             long log_steps, long* state_host);

/* MD observers behind a resident MD driver's finish (added within ABI v13: new entry points only; hermnet_amd/observe.py:
 * Frames, MSD, RDF; csrc/observe_kernels.hip, observe_step.h).  Launched behind the driver's commit kernel, so they read the
 * NEW state.  Each observer owns obs [4] int64 = (last sampled step, samples taken, reserved, reserved), obs[0] = -1 at the
 * start.  A sample is DUE iff state[1] == 0 and state[0] % stride == 0 and state[0] > obs[0]: the prime of a construction
 * samples the start configuration as step 0; void steps, halted and parked replays and the prime behind a resume sample
 * nothing.  Not due: nothing is written.  Each call is its worker launch and one single-workgroup launch that alone writes obs
 * (obs[0] = step, obs[1] += 1) and the ring's steps[slot].  No float atomics; the counts and sums are reproducible bit for bit.
 *
 * hermnet_observe_frames  slot = obs[1] % frames:  positions[slot,i,:] = float(x[i,:]);  velocities[slot] = float(v) and
 *   images[slot] = image where given (v / velocities and image / images are NULL together);  cells[slot] = cell [B,3,3], the
 *   step's float32 cell (NULL: open structures);  steps[slot] = step.
 * hermnet_observe_msd     species [N] int32 in [0, num_species).  The first sample stores x_origin, image_origin = x, image.
 *   d = (x - x_origin) + (image - image_origin) cell, with the current float32 cell widened (cell NULL: d = x - x_origin);
 *   sums[slot,g,s,:] = (sum d_x, sum d_y, sum d_z, sum |d|^2) over the atoms of species s of graph g in float64 in
 *   hermnet_md_finish's fixed order, atoms of other species skipped in place;  slot = obs[1] % rows;  steps[slot] = step.
 * hermnet_observe_rdf     per atom s_k = (x0 inv[k] + x1 inv[3+k]) + x2 inv[6+k];  per pair i < j of one graph ds = s_i - s_j,
 *   ds -= floor(ds + 0.5), d = ds cell as (a + b) + c, r2 = (d0^2 + d1^2) + d2^2, all float64 (cell and inv_cell NULL: s = x,
 *   d = ds).  The pair counts in bin b iff edge2[b] <= r2 < edge2[b+1] (edge2 [bins+1] ascending from 0, made by the caller),
 *   once, in counts[slot, p, b] with p = a S - a (a - 1) / 2 + (b' - a) for its species a <= b' of S = num_species, and
 *   slot = slot_of[g] (clamped to [0, slots)) or g where slot_of is NULL.  A graph with r_max2 |column k of inv_cell|^2 > 1/4
 *   for some k -- the rounding is the minimum image only below half the smallest cell height -- is not counted in that
 *   sample: skipped[slot] += 1; otherwise samples[slot] += 1 and volume_sum[slot] += |det cell|, in the order of the graphs.
 *   work [num_work,3] int32 = (graph, tile_i, tile_j >= tile_i) over 256-atom tiles of every graph, made by the caller; one
 *   256-lane workgroup per entry, a uint32 histogram in LDS, integer atomic adds of its nonzero bins to counts.
 * The hermnet_host_observe_* twins run the same text on HOST pointers (no stream): the same integers and the same bits.
 * HN_ERR_BAD_ARG: a NULL pointer that is needed, num_graphs < 1, stride < 1, frames / rows / slots < 1, num_species < 1,
 *   bins < 1 or > 1024, num_species (num_species + 1) / 2 x bins > 8192, r_max2 <= 0, slots < num_graphs without slot_of; the
 *   host twin also refuses a work list that names a graph that does not exist or tile_j < tile_i. */
int hermnet_observe_frames(int num_atoms, int num_graphs, long stride, long frames, const double* x, const double* v,
                           const int* image, const float* cell, const long* state, long* obs, long* steps, float* positions,
                           float* velocities, int* images, float* cells, void* stream);
int hermnet_observe_msd(int num_atoms, int num_graphs, int num_species, long stride, long rows, const int* graph_ptr,
                        const int* species, const double* x, const int* image, const float* cell, const long* state, long* obs,
                        long* steps, double* x_origin, int* image_origin, double* sums, void* stream);
int hermnet_observe_rdf(int num_atoms, int num_graphs, int num_species, int bins, long slots, long stride, double r_max2,
                        const int* graph_ptr, const int* species, const double* x, const float* cell, const double* inv_cell,
                        const long* slot_of, const double* edge2, const int* work, int num_work, const long* state, long* obs,
                        long* counts, long* samples, long* skipped, double* volume_sum, void* stream);
int hermnet_host_observe_frames(int num_atoms, int num_graphs, long stride, long frames, const double* x_host,
                                const double* v_host, const int* image_host, const float* cell_host, const long* state_host,
                                long* obs_host, long* steps_host, float* positions_host, float* velocities_host,
                                int* images_host, float* cells_host);
int hermnet_host_observe_msd(int num_atoms, int num_graphs, int num_species, long stride, long rows, const int* graph_ptr_host,
                             const int* species_host, const double* x_host, const int* image_host, const float* cell_host,
                             const long* state_host, long* obs_host, long* steps_host, double* x_origin_host,
                             int* image_origin_host, double* sums_host);
int hermnet_host_observe_rdf(int num_atoms, int num_graphs, int num_species, int bins, long slots, long stride, double r_max2,
                             const int* graph_ptr_host, const int* species_host, const double* x_host, const float* cell_host,
                             const double* inv_cell_host, const long* slot_of_host, const double* edge2_host,
                             const int* work_host, int num_work, const long* state_host, long* obs_host, long* counts_host,
                             long* samples_host, long* skipped_host, double* volume_sum_host);

/* Multiple-walker metadynamics inside the replayed MD step (added within ABI v13: new entry points only;
 * hermnet_amd/metad.py: DeviceMetaD; csrc/metad_kernels.hip, metad_step.h).  A stage of four launches between the force
 * backward and the UNCHANGED hermnet_md_finish, which is handed forces_b in the place of the step's forces.  The B graphs are B
 * walkers of ONE system of n_rep = N / B atoms (walker g: rows g n_rep .. (g + 1) n_rep) under one shared bias
 *   V(s) = sum_k hill_heights[k] prod_d E(-(s_d - hill_centres[k,d])^2 / (2 sigma_d^2)),   k < hill_count[0],
 * E = the library's own exp (range reduction by ln 2 in two parts, a Horner polynomial of degree 13 on |r| <= ln 2 / 2,
 * ldexp; 0 below -745), the same bits on the device and on the host.  The cell is fixed and periodic.
 *
 * D = num_cvs = 1 or 2 collective variables, every table made on the host:  cv_kind [D,2] int32 = (kind, p);  cv_par [D,8]
 * float64;  cv_role [D,n_rep] bytes;  cv_weight [D,2,n_rep] float64;  sigma_par [D,2] = (1 / (2 sigma^2), 1 / sigma^2).
 *   kind 1, distance:  centre a = sum_i cv_weight[d,0,i] u_i, centre b likewise with cv_weight[d,1,:] (normalised weights, 0
 *     outside a group), u_i = x_i + image_i cell the UNWRAPPED coordinate, the sums in hermnet_md_finish's fixed order;
 *     s = |minimum image of (a - b)| by hermnet_observe_rdf's rule, ds/dx_i = (wa_i - wb_i) (a - b) / s, 0 at s = 0.
 *   kind 2, coordination:  s = scale sum_{i in A} sum_{j in B, j != i} st(r_ij), cv_role bit 0 = in A, bit 1 = in B;
 *     w = r^2 cv_par[0], sw = 1 / (1 + w^p) with w^p by multiplications, st = (sw - cv_par[2]) cv_par[3] for r^2 < cv_par[1]
 *     and 0 beyond;  cv_par = (1 / r0^2, r_cut^2, sw(w_c), 1 / (1 - sw(w_c)), 2 cv_par[3] / r0^2, scale, 0, 0).  Every atom
 *     sums its own count and its own gradient over all partners j of its walker in ascending j (minimum image as above):
 *     no atomics, nothing scattered.
 * Caller-owned state:  hill_count [1] int64, hill_centres [max_hills,D], hill_heights [max_hills] float64;  scratch cv_atom
 * [D,N,6] and cv_walker [B,16] float64 (row g = s_0, s_1, V, dV/ds_0, dV/ds_1, height, ...);  forces_b [N,3] float32;
 * bias_forces [N,3] float64;  cv_log [log_steps,B,D+2] float64.
 *
 * hermnet_metad_bias     state[1] != 0: nothing.  Otherwise the step's halt code is formed from energy / total / capacity as
 *   hermnet_md_finish forms it.  Code != 0: forces_b = forces, nothing else.  Code 0: per walker s, V(s) and dV/ds over the
 *   hills counted when the step began (hill index in hermnet_md_finish's fixed order);  per atom nb = sum_d dV/ds_d ds_d/dx_i
 *   from 0.0, bias_forces = -nb, forces_b = (float)((double)forces - nb).  Mode 0 (state[3] == 0) also writes
 *   cv_log[state[0] % log_steps][g] = (s_1..s_D, V(s), height deposited or 0), and where (state[0] + 1) % pace == 0 walker g
 *   appends the hill (s, h) at hill_count + g, h = height, or height E(-V(s) inv_kt) where inv_kt = 1 / (kB (gamma - 1) T)
 *   is not 0;  hill_count += B, never beyond max_hills.  One workgroup alone writes the hill list and its count.
 * hermnet_metad_cv       the per-atom pass and the CV sums alone:  values [B,D], grads [D,N,3] = ds_d/dx_i.
 * hermnet_host_metad_exp out[i] = E(a[i]).
 * The hermnet_host_metad_* twins run the same text on HOST pointers (no stream), bit for bit what the device computes.
 * HN_ERR_BAD_ARG: a NULL pointer, num_graphs < 1, num_cvs not 1 or 2, num_atoms no multiple of num_graphs, pace / max_hills /
 *   log_steps < 1;  the host twins also refuse walkers that do not tile the atoms in equal ranges, a kind other than 1 or 2
 *   and a power outside 1..64. */
int hermnet_metad_bias(int num_atoms, int num_graphs, int num_cvs, const int* graph_ptr, const double* x, const int* image,
                       const float* cell, const double* inv_cell, const int* cv_kind, const double* cv_par,
                       const unsigned char* cv_role, const double* cv_weight, const double* sigma_par, double height,
                       double inv_kt, long pace, long max_hills, const float* forces, const float* energy, const long* total,
                       long capacity, const long* state, double* cv_atom, double* cv_walker, long* hill_count,
                       double* hill_centres, double* hill_heights, float* forces_b, double* bias_forces, double* cv_log,
                       long log_steps, void* stream);
int hermnet_metad_cv(int num_atoms, int num_graphs, int num_cvs, const int* graph_ptr, const double* x, const int* image,
                     const float* cell, const double* inv_cell, const int* cv_kind, const double* cv_par,
                     const unsigned char* cv_role, const double* cv_weight, double* cv_atom, double* cv_walker, double* values,
                     double* grads, void* stream);
int hermnet_host_metad_bias(int num_atoms, int num_graphs, int num_cvs, const int* graph_ptr_host, const double* x_host,
                            const int* image_host, const float* cell_host, const double* inv_cell_host, const int* cv_kind_host,
                            const double* cv_par_host, const unsigned char* cv_role_host, const double* cv_weight_host,
                            const double* sigma_par_host, double height, double inv_kt, long pace, long max_hills,
                            const float* forces_host, const float* energy_host, const long* total_host, long capacity,
                            const long* state_host, double* cv_atom_host, double* cv_walker_host, long* hill_count_host,
                            double* hill_centres_host, double* hill_heights_host, float* forces_b_host,
                            double* bias_forces_host, double* cv_log_host, long log_steps);
int hermnet_host_metad_cv(int num_atoms, int num_graphs, int num_cvs, const int* graph_ptr_host, const double* x_host,
                          const int* image_host, const float* cell_host, const double* inv_cell_host, const int* cv_kind_host,
                          const double* cv_par_host, const unsigned char* cv_role_host, const double* cv_weight_host,
                          double* cv_atom_host, double* cv_walker_host, double* values_host, double* grads_host);
int hermnet_host_metad_exp(long n, const double* a_host, double* out_host);

/* Species-swap Monte Carlo inside the replayed MD step (added within ABI v13: new entry points only; hermnet_amd/swapmc.py:
 * DeviceSwapMD; csrc/swapmc_kernels.hip, swapmc_step.h).  hermnet_swapmc_advance stands in the place of hermnet_md_advance in
 * front of the search, hermnet_swapmc_finish in the place of hermnet_md_finish behind the force backward.  In a fixed
 * composition, exchanging the species of two atoms is exchanging their coordinates: z, masses, velocities and every per-atom
 * table stay with their rows.
 *
 * Caller-owned state beside hermnet_md_advance's / _finish's:  mc [2] int64 = (t, left), the trials committed so far and the
 * trials still due in this block;  cand [num_cand] int32, per graph its atoms of finite mass sorted by (species, atom), and
 * cand_ptr [B, S+1] int32, the absolute offsets of each species' range in cand (S = num_species);  beta [B] float64 =
 * 1 / (kB T);  e_ref [B] float64 the energy of the current configuration;  attempts, accepts [B] int64;  swap_log
 * [swap_rows,B,4] float64;  scratch: pair [B,2] int32, dval [B] float64, outcome [B] int64.  `seed` is hermnet_md_advance's.
 *
 * With the words as the replay begins: halt code != 0: nothing.  state[3] == 1: a PRIME -- hermnet_md_advance's and
 * hermnet_md_finish's, and e_ref = energy; mc untouched.  Otherwise left > 0: a TRIAL; otherwise an MD STEP --
 * hermnet_md_advance's and hermnet_md_finish's (the log row's E_kin in the canonical order), and e_ref = energy; where the
 * new step % swap_interval == 0, left = swaps.
 * A trial, graph g:  w = Philox4x32-10 of key (seed low, seed high), counter (g, t low, t high, 3);  m = the graph's
 *   candidates, mulhi(w, m) = ((uint64)w * m) >> 32;  i = cand[ptr[0] + mulhi(w0, m)], s its species with m_s candidates;
 *   k = mulhi(w1, m - m_s), q = k < ptr[s] - ptr[0] ? k : k + m_s, j = cand[ptr[0] + q];  m - m_s == 0: not tried.
 *   hermnet_swapmc_advance exchanges x and image of (i, j) and writes their pos32 rows; nothing else.
 *   hermnet_swapmc_finish:  d = (double)energy[g] - e_ref[g];  delta = -beta[g] d;  accepted iff delta >= 0 or log(u) < delta,
 *   u = (u(w2,w3) + 1) 2^-53 with hermnet_md_advance's u(,).  Accepted: f_prev of g's atoms = forces, e_ref[g] = energy[g].
 *   Rejected: (i, j) exchanged back.  swap_log[t % swap_rows][g] = (i, j, d, outcome: 0 not tried, 1 rejected, 2 accepted;
 *   not tried: -1, -1, 0, 0);  attempts[g] counts tried, accepts[g] accepted trials;  t += 1, left -= 1.  The step's code
 *   != 0: the trial is void -- every pair exchanged back, state = (step, code, step, 0), mc and every record untouched.
 *   A trial writes no velocity, no MD log row, and leaves state[0].
 *   One launch in the advance, four in the finish: one workgroup with a lane per graph that writes the scratch alone; the
 *   per-atom launch; one workgroup per graph (an MD step's log row); and the one workgroup that alone writes e_ref, the
 *   counters, swap_log, mc and state.  No atomics; no workgroup reads what another of the same launch writes.
 * The hermnet_host_swapmc_* twins run the same text on HOST pointers (no stream), bit for bit but for the last digits of
 * log(u) and of the atoms' Gaussians.
 * HN_ERR_BAD_ARG: hermnet_md_advance's / _finish's, a NULL pointer (cand may be NULL with num_cand == 0), num_species < 1,
 *   num_cand < 0, swap_interval < 1, swaps < 0, swap_rows < 1; the host twins also refuse a negative mc word, species ranges
 *   that do not ascend inside cand and a candidate that is no atom of its graph or does not ascend within its species (the
 *   device entry points cannot read them: there such a graph is not tried). */
int hermnet_swapmc_advance(int num_atoms, int num_graphs, int flags, double dt, unsigned long seed, double* x, double* v,
                           double* x0, double* v0, int* image, int* image0, const float* f_prev, const double* kick,
                           const double* c1, const double* sigma, const long* batch, const float* cell, const double* inv_cell,
                           float* pos32, const long* state, const long* mc, const int* graph_ptr, const int* cand,
                           const int* cand_ptr, int num_species, int num_cand, void* stream);
int hermnet_swapmc_finish(int num_atoms, int num_graphs, const int* graph_ptr, const long* batch, const float* forces,
                          const float* energy, const long* total, long capacity, long swap_interval, long swaps,
                          unsigned long seed, double* x, double* v, const double* x0, const double* v0, int* image,
                          const int* image0, float* f_prev, const double* kick, const double* half_mass, float* pos32,
                          double* ke_atom, const double* beta, double* e_ref, long* mc, const int* cand, const int* cand_ptr,
                          int num_species, int num_cand, int* pair, double* dval, long* outcome, long* attempts, long* accepts,
                          double* swap_log, long swap_rows, double* log, long log_steps, long* state, void* stream);
int hermnet_host_swapmc_advance(int num_atoms, int num_graphs, int flags, double dt, unsigned long seed, double* x_host,
                                double* v_host, double* x0_host, double* v0_host, int* image_host, int* image0_host,
                                const float* f_prev_host, const double* kick_host, const double* c1_host,
                                const double* sigma_host, const long* batch_host, const float* cell_host,
                                const double* inv_cell_host, float* pos32_host, const long* state_host, const long* mc_host,
                                const int* graph_ptr_host, const int* cand_host, const int* cand_ptr_host, int num_species,
                                int num_cand);
int hermnet_host_swapmc_finish(int num_atoms, int num_graphs, const int* graph_ptr_host, const long* batch_host,
                               const float* forces_host, const float* energy_host, const long* total_host, long capacity,
                               long swap_interval, long swaps, unsigned long seed, double* x_host, double* v_host,
                               const double* x0_host, const double* v0_host, int* image_host, const int* image0_host,
                               float* f_prev_host, const double* kick_host, const double* half_mass_host, float* pos32_host,
                               double* ke_atom_host, const double* beta_host, double* e_ref_host, long* mc_host,
                               const int* cand_host, const int* cand_ptr_host, int num_species, int num_cand, int* pair_host,
                               double* dval_host, long* outcome_host, long* attempts_host, long* accepts_host,
                               double* swap_log_host, long swap_rows, double* log_host, long log_steps, long* state_host);

/* Nose-Hoover chain NVT inside the replayed MD step (added within ABI v13: new entry points only; hermnet_amd/nhc.py:
 * DeviceNHC; csrc/nhc_kernels.hip, nhc_step.h).  hermnet_nhc_advance stands in the place of hermnet_md_advance in front of
 * the search, hermnet_nhc_finish in the place of hermnet_md_finish behind the force backward; a time step is
 * NHC(dt/2) kick(dt/2) drift(dt) [forces] kick(dt/2) NHC(dt/2) with hermnet_md_advance's NVE kick, drift and wrap and
 * hermnet_md_finish's kick, void step and commit.  `flags`: hermnet_md_advance's without HN_MD_LANGEVIN.
 *
 * Caller-owned state beside hermnet_md_advance's / _finish's, all float64:  xi, v_xi [B,M] the chains (M = chain, 1..8);
 * xi0, v_xi0 [B,M] their backup;  scale [B,2] the last opening and closing factor;  constants made on the host:  delta
 * [order] = w_k (dt / 2) / substeps for the Suzuki-Yoshida weights w (order 1, 3 or 5),  kt [B] = kB T,  dof_kt [B] = dof kB T,
 * q [B,M] = (dof kB T tau^2, kB T tau^2, ...) and inv_q [B,M] = 1 / q -- both 0 for a graph whose thermostat is off.
 *
 * NHC(Delta) of graph g (Martyna, Tuckerman, Tobias, Klein 1996): K2 = 2 E_kin, s = 1; substeps times, for every weight, with
 * d = delta[k]:  v_M += G_M d/2;  j = M-1..1: e = exp(-d/4 v_{j+1}), v_j = (v_j e + G_j d/2) e;  a = exp(-d v_1), s = s a,
 * K2 = (K2 a) a;  xi_j += d v_j;  j = 1..M-1: the same update with G_j made anew;  v_M += G_M d/2.  G_1 = (K2 - dof_kt)
 * inv_q_1, G_j = (q_{j-1} v_{j-1}^2 - kt) inv_q_j.  exp is the library's own (hermnet_host_metad_exp): IEEE +, x, floor and
 * ldexp alone, contraction off, so device, host twin and a numpy transcription agree bit for bit; with inv_q = q = v_xi = 0
 * every factor is exactly 1.0 and the step is hermnet_md_advance's / _finish's NVE bit for bit.
 *
 * hermnet_nhc_advance (no halt code, state[3] == 0; a prime only rewrites pos32 as hermnet_md_advance does): per graph E_kin =
 *   sum half_mass |v|^2 in the canonical order from v as it stands (not a number the last finish left), (xi0, v_xi0) =
 *   (xi, v_xi), NHC(dt/2), scale[g][0] = s; per atom v0 = v (unscaled), v = v s, then hermnet_md_advance's NVE step.
 * hermnet_nhc_finish: hermnet_md_finish's per-atom half; on a step that commits per graph the canonical E_kin = K behind the
 *   second kick, NHC(dt/2), scale[g][1] = s, log row (width 4) = (energy[g], (K s) s, total[0], E_nhc),
 *   E_nhc = dof_kt xi_1 + kt sum_{j>=2} xi_j + sum_j q_j v_j^2 / 2;  per atom v = v s;  on a void step (xi, v_xi) = (xi0, v_xi0)
 *   beside hermnet_md_finish's restore;  then hermnet_md_finish's commit.  Two launches in the advance, four in the finish,
 *   no atomics; no workgroup reads what another of the same launch writes.
 * The hermnet_host_nhc_* twins run the same text on HOST pointers (no stream), bit for bit.
 * HN_ERR_BAD_ARG: hermnet_md_advance's / _finish's, HN_MD_LANGEVIN in flags, chain outside 1..8, order not 1, 3 or 5,
 *   substeps < 1, a NULL pointer (batch may be NULL: one graph). */
int hermnet_nhc_advance(int num_atoms, int num_graphs, int flags, double dt, double* x, double* v, double* x0, double* v0,
                        int* image, int* image0, const float* f_prev, const double* kick, const long* batch, const float* cell,
                        const double* inv_cell, float* pos32, const long* state, const int* graph_ptr, const double* half_mass,
                        int chain, int order, int substeps, const double* delta, const double* kt, const double* dof_kt,
                        const double* q, const double* inv_q, double* xi, double* v_xi, double* xi0, double* v_xi0,
                        double* scale, void* stream);
int hermnet_nhc_finish(int num_atoms, int num_graphs, const int* graph_ptr, const long* batch, const float* forces,
                       const float* energy, const long* total, long capacity, double* x, double* v, const double* x0,
                       const double* v0, int* image, const int* image0, float* f_prev, const double* kick,
                       const double* half_mass, float* pos32, double* ke_atom, int chain, int order, int substeps,
                       const double* delta, const double* kt, const double* dof_kt, const double* q, const double* inv_q,
                       double* xi, double* v_xi, double* xi0, double* v_xi0, double* scale, double* log, long log_steps,
                       long* state, void* stream);
int hermnet_host_nhc_advance(int num_atoms, int num_graphs, int flags, double dt, double* x_host, double* v_host,
                             double* x0_host, double* v0_host, int* image_host, int* image0_host, const float* f_prev_host,
                             const double* kick_host, const long* batch_host, const float* cell_host,
                             const double* inv_cell_host, float* pos32_host, const long* state_host,
                             const int* graph_ptr_host, const double* half_mass_host, int chain, int order, int substeps,
                             const double* delta_host, const double* kt_host, const double* dof_kt_host, const double* q_host,
                             const double* inv_q_host, double* xi_host, double* v_xi_host, double* xi0_host,
                             double* v_xi0_host, double* scale_host);
int hermnet_host_nhc_finish(int num_atoms, int num_graphs, const int* graph_ptr_host, const long* batch_host,
                            const float* forces_host, const float* energy_host, const long* total_host, long capacity,
                            double* x_host, double* v_host, const double* x0_host, const double* v0_host, int* image_host,
                            const int* image0_host, float* f_prev_host, const double* kick_host,
                            const double* half_mass_host, float* pos32_host, double* ke_atom_host, int chain, int order,
                            int substeps, const double* delta_host, const double* kt_host, const double* dof_kt_host,
                            const double* q_host, const double* inv_q_host, double* xi_host, double* v_xi_host,
                            double* xi0_host, double* v_xi0_host, double* scale_host, double* log_host, long log_steps,
                            long* state_host);

/* Nose-Hoover (MTK) barostat NPT inside the replayed MD step (added within ABI v13: new entry points only; hermnet_amd/mtk.py:
 * DeviceMTK; csrc/mtk_kernels.hip, mtk_step.h -- the definition of the step, operation by operation, is that header's).
 * hermnet_mtk_advance stands in the place of hermnet_md_advance in front of the search and moves the cell before the search
 * reads it; hermnet_mtk_finish stands in the place of hermnet_md_finish_npt behind the force backward and the virial.  The
 * integrator is the measure-preserving, reversible MTK splitting of Tuckerman et al. (J. Phys. A 39, 5629 (2006)):
 *   NHC_baro NHC_particles baro-kick | scaled kick, scaled drift, cell | [forces, virial] | scaled kick | baro-kick NHC_particles
 *   NHC_baro,  every half of length dt / 2.  `flags`: hermnet_md_advance's without HN_MD_LANGEVIN.
 *
 * Caller-owned state beside hermnet_nhc_advance's / _finish's (the particles' chain: the 13 arguments chain ... scale):
 *   coupling  HN_MD_BARO_ISOTROPIC (mask must be 7) or HN_MD_BARO_AXES (mask: bit a = Cartesian axis a is coupled, not 0)
 *   max_strain  in (0, 0.1]: the largest |v_g,a| dt of a step that is not refused
 *   par [B,5] float64 = (w, 1 / w, 1 + 3 / dof, 1 / dof, P0) with the barostat's mass w = (dof + 3) kB T taup^2 (isotropic) or a
 *     third of that per axis; taup = inf: w = 1 / w = 0 and the barostat never moves
 *   dof_kt_b [B], q_b, inv_q_b [B,M]  the barostat chain's tables (dof_b = 1 or the number of coupled axes; Q_1 = dof_b kB T
 *     taup^2, Q_j = kB T taup^2; both 0 where tau = inf or taup = inf);  xi_b, v_xi_b [B,M] that chain, scale_b [B,2] its last
 *     opening and closing factor
 *   v_cell [B,3]  the diagonal of the cell's rate in Cartesian axes (isotropic: three times one number)
 *   cell64 [B,9] float64 (the truth), cell32 [B,9] float32 (its rounding: what the search reads), inv_cell [B,9] float64 (the
 *     adjugate inverse of the widened cell32; unwritten while the cell does not move)
 *   w_prev [B,9] float32  the virial of the last accepted evaluation (P = (sum m v v + sym W) / V)
 *   factors [B,12]  scratch: a[3], b[3] (the kicks'), rx[3], rv[3] (the drift's) of the step
 *   backup [B,2M+30]  xi_b, v_xi_b, v_cell, cell64, cell32 (widened), inv_cell at the start of the step
 *   flag [B] int64  1: this step's factors were refused (|v_g,a| dt > max_strain, or a factor that is not finite) -- identity
 *     factors are used, the cell stays, and the finish voids the step;  refused [B] int64: how often
 *   e_code [B] float32  scratch: what the commit kernel reads as the energies (NaN where the barostat voids the step)
 * hermnet_mtk_finish: `virial` [B,9] float32 is the step's own.  Its code is hermnet_md_finish's | HN_MD_HALT_NONFINITE where a
 *   graph is flagged or a virial entry is not finite; void: atoms, v_cell, both chains and the three forms of the cell return,
 *   no row.  Log row (width 7) = (energy[g], E_kin behind the closing factor, total[0], E_nhc of both chains, tr P / 3 at the
 *   end of the step, volume, P0 V + w sum_coupled v_cell^2 / 2); columns 0 + 1 + 3 + 6 are conserved.  mode 1 (a prime): f_prev =
 *   forces and w_prev = virial where the code is 0, nothing else.  Two launches in the advance, four in the finish, no atomics.
 * The hermnet_host_mtk_* twins run the same text on HOST pointers (no stream), bit for bit.
 * HN_ERR_BAD_ARG: hermnet_nhc_advance's / _finish's, dt <= 0, a coupling other than the two, a mask that is 0, has bits above 7
 *   or is not 7 under isotropic coupling, max_strain outside (0, 0.1], a NULL pointer (batch may be NULL: one graph). */
int hermnet_mtk_advance(int num_atoms, int num_graphs, int flags, double dt, double* x, double* v, double* x0, double* v0,
                        int* image, int* image0, const float* f_prev, const double* kick, const long* batch, float* pos32,
                        const long* state, const int* graph_ptr, const double* half_mass, int chain, int order, int substeps,
                        const double* delta, const double* kt, const double* dof_kt, const double* q, const double* inv_q,
                        double* xi, double* v_xi, double* xi0, double* v_xi0, double* scale, int coupling, int mask,
                        double max_strain, const double* par, const double* dof_kt_b, const double* q_b, const double* inv_q_b,
                        double* xi_b, double* v_xi_b, double* scale_b, double* v_cell, double* cell64, float* cell32,
                        double* inv_cell, float* w_prev, double* factors, double* backup, long* flag, long* refused,
                        float* e_code, void* stream);
int hermnet_mtk_finish(int num_atoms, int num_graphs, const int* graph_ptr, const long* batch, const float* forces,
                       const float* energy, const float* virial, const long* total, long capacity, double dt, double* x,
                       double* v, const double* x0, const double* v0, int* image, const int* image0, float* f_prev,
                       const double* kick, const double* half_mass, float* pos32, double* ke_atom, int chain, int order,
                       int substeps, const double* delta, const double* kt, const double* dof_kt, const double* q,
                       const double* inv_q, double* xi, double* v_xi, double* xi0, double* v_xi0, double* scale, int coupling,
                       int mask, double max_strain, const double* par, const double* dof_kt_b, const double* q_b,
                       const double* inv_q_b, double* xi_b, double* v_xi_b, double* scale_b, double* v_cell, double* cell64,
                       float* cell32, double* inv_cell, float* w_prev, double* factors, double* backup, long* flag,
                       long* refused, float* e_code, double* log, long log_steps, long* state, void* stream);
int hermnet_host_mtk_advance(int num_atoms, int num_graphs, int flags, double dt, double* x_host, double* v_host,
                             double* x0_host, double* v0_host, int* image_host, int* image0_host, const float* f_prev_host,
                             const double* kick_host, const long* batch_host, float* pos32_host, const long* state_host,
                             const int* graph_ptr_host, const double* half_mass_host, int chain, int order, int substeps,
                             const double* delta_host, const double* kt_host, const double* dof_kt_host, const double* q_host,
                             const double* inv_q_host, double* xi_host, double* v_xi_host, double* xi0_host,
                             double* v_xi0_host, double* scale_host, int coupling, int mask, double max_strain,
                             const double* par_host, const double* dof_kt_b_host, const double* q_b_host,
                             const double* inv_q_b_host, double* xi_b_host, double* v_xi_b_host, double* scale_b_host,
                             double* v_cell_host, double* cell64_host, float* cell32_host, double* inv_cell_host,
                             float* w_prev_host, double* factors_host, double* backup_host, long* flag_host,
                             long* refused_host, float* e_code_host);
int hermnet_host_mtk_finish(int num_atoms, int num_graphs, const int* graph_ptr_host, const long* batch_host,
                            const float* forces_host, const float* energy_host, const float* virial_host,
                            const long* total_host, long capacity, double dt, double* x_host, double* v_host,
                            const double* x0_host, const double* v0_host, int* image_host, const int* image0_host,
                            float* f_prev_host, const double* kick_host, const double* half_mass_host, float* pos32_host,
                            double* ke_atom_host, int chain, int order, int substeps, const double* delta_host,
                            const double* kt_host, const double* dof_kt_host, const double* q_host, const double* inv_q_host,
                            double* xi_host, double* v_xi_host, double* xi0_host, double* v_xi0_host, double* scale_host,
                            int coupling, int mask, double max_strain, const double* par_host, const double* dof_kt_b_host,
                            const double* q_b_host, const double* inv_q_b_host, double* xi_b_host, double* v_xi_b_host,
                            double* scale_b_host, double* v_cell_host, double* cell64_host, float* cell32_host,
                            double* inv_cell_host, float* w_prev_host, double* factors_host, double* backup_host,
                            long* flag_host, long* refused_host, float* e_code_host, double* log_host, long log_steps,
                            long* state_host);

#ifdef __cplusplus
}
#endif
#endif /* HERMNET_HIP_H */
