/*
 * neuma_hip.h — C ABI of libneuma_hip.so, the MI355X (gfx950) engine behind NeuMA's
 * simulator / constitutive-net / Particle-GS render operators.
 *
 * The reference (XJay18/NeuMA) has no C ABI of its own: it reaches the GPU through Warp's JIT
 * (`wp.launch`) and through the pybind11 torch extension `diff_gaussian_rasterization`.
 * Each entry point below names the reference interface it replaces (file:line relative to the
 * reference root).  INTEGRATION.md shows the ctypes binding a NeuMA maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into memory owned by the caller (PyTorch); the library
 *     borrows it for the duration of the call and never frees or retains it.  Exceptions: the
 *     opaque handles, which own their scratch (grid, active-block lists), and `*_cfg` structs
 *     and `int* out` scalars, which are HOST pointers.
 *   - fp32, contiguous, array-of-structures exactly as torch lays them out:
 *     x,v (N,3); C,F,stress (N,3,3) row-major; statics float/int32 (N,); cov6 order
 *     xx,xy,xz,yy,yz,zz; SH (K, M, 3); view/proj matrices 16 floats in torch row-major order of
 *     the (already transposed, row-vector convention) tensors NeuMA passes.
 *   - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream).  All calls are
 *     asynchronous on that stream unless stated; no device-wide synchronisation is issued.
 *   - return 0 on success, negative on error; nm_last_error() gives the thread-local message.
 *     Non-finite gradients are not an error (the Python shim applies nan_to_num like
 *     modules/nclaw/sim/interface.py:65-74).
 *   - a handle is not thread-safe; different handles may be used concurrently.
 */
#ifndef NEUMA_HIP_H
#define NEUMA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NM_OK 0
#define NM_ERR_INVALID (-1)
#define NM_ERR_HIP (-2)
#define NM_ERR_WORKSPACE (-3)
#define NM_ERR_LIMIT (-4) /* an iteration limit given by the caller was reached (nm_emd) */

int nm_version(void);
const char* nm_last_error(void);

/* ------------------------------------------------------------------ in-library kernel timing (bench.py roofline) */

/* HIP-event timing of the library's own kernel launches, on the stream they are launched on.
 * nm_prof_enable(1, NULL) times every kernel; nm_prof_enable(1, "k_render_bwd") only that one (two event
 * records per launch); nm_prof_enable(n > 1, name) times every n-th matching launch only (a pair of event records costs
 * ~11 us of bubble around the launch: sampling keeps a timed region honest); nm_prof_enable(0, NULL) stops.  nm_prof_report synchronises the recorded events and
 * writes "name calls total_ms\n" lines (NUL-terminated, truncated to cap); nm_prof_reset drops the samples. */
int nm_prof_enable(int32_t on, const char* only_kernel);
int nm_prof_report(char* out, size_t cap);
int nm_prof_reset(void);

/* ------------------------------------------------------------------ MPM (modules/nclaw/sim) */

/* MPMConstant, modules/nclaw/sim/mpm.py:158-167; parse_cfg 507-528 (dx = 1/num_grids). */
typedef struct nm_mpm_cfg {
  int32_t num_grids;
  float dt;
  int32_t bound;
  float gravity[3];
  float eps;
  int32_t bc; /* 0 = noslip (mpm.py:402-429), 1 = freeslip (mpm.py:373-400) */
} nm_mpm_cfg;

/* MPMStatics, mpm.py:14-72 */
typedef struct nm_statics {
  const float* vol;
  const float* rho;
  const float* clip_bound;
  const int32_t* enabled;
} nm_statics;

/* MPMParticleData, mpm.py:75-128 (values or gradients; unused members may be NULL) */
typedef struct nm_particles {
  float* x;      /* (N,3)   */
  float* v;      /* (N,3)   */
  float* C;      /* (N,3,3) */
  float* F;      /* (N,3,3) */
  float* stress; /* (N,3,3) */
} nm_particles;

typedef struct nm_mpm nm_mpm; /* MPMModel (mpm.py:245-258): owns the grid */

/* MPMModelBuilder.finalize, mpm.py:543-551.  bc outside {0,1} -> NM_ERR_INVALID (ValueError there). */
int nm_mpm_create(const nm_mpm_cfg* cfg, nm_mpm** out);
int nm_mpm_destroy(nm_mpm* h);

/* MPMModel.forward, mpm.py:279-297: grid clear, p2g, grid_op, g2p.  `next` may alias `cur`
 * (MPMForwardSim, interface.py:131-135).  Writes next->x,v,C,F. */
int nm_mpm_forward(nm_mpm* h, int32_t n, const nm_statics* st, const nm_particles* cur,
                   nm_particles* next, void* stream);

/* MPMModel.backward, mpm.py:299-319: recompute p2g + grid_op, then the adjoints of g2p,
 * grid_op, p2g.  gnext: incoming dL/d(x,v,C,F) of the next state (stress ignored);
 * gcur: outgoing dL/d(x,v,C,F,stress) of the current state (overwritten).
 * `next` holds the forward outputs of this step (v, C are read). */
int nm_mpm_backward(nm_mpm* h, int32_t n, const nm_statics* st, const nm_particles* cur,
                    const nm_particles* next, const nm_particles* gnext, nm_particles* gcur,
                    void* stream);

/* Grid cache (no reference counterpart; removes the reference's p2g recompute of mpm.py:312-315 from the reverse
 * sweep).  nm_mpm_forward_ex additionally writes a record of the substep's touched 4x4x4-node blocks ({mv, m} of
 * those blocks + the block list; nm_mpm_gridcache_bytes(cap_blocks) bytes, caller-owned device memory);
 * nm_mpm_backward_ex restores the grid from it instead of re-scattering.  A substep that touches more than
 * cap_blocks blocks marks its record invalid and the backward transparently falls back to the recompute, so results
 * never depend on the capacity.  gridrec == NULL: identical to nm_mpm_forward / nm_mpm_backward. */
size_t nm_mpm_gridcache_bytes(int32_t cap_blocks);
int nm_mpm_forward_ex(nm_mpm* h, int32_t n, const nm_statics* st, const nm_particles* cur,
                      nm_particles* next, void* gridrec, int32_t cap_blocks, void* stream);
int nm_mpm_backward_ex(nm_mpm* h, int32_t n, const nm_statics* st, const nm_particles* cur,
                       const nm_particles* next, const nm_particles* gnext, nm_particles* gcur,
                       const void* gridrec, int32_t cap_blocks, void* stream);

/* MPMModel.forward_extra, mpm.py:260-277: p2g + grid_op from (st, cur), then g2p of a second,
 * passive particle set in place. */
int nm_mpm_forward_extra(nm_mpm* h, int32_t n, const nm_statics* st, const nm_particles* cur,
                         int32_t n_extra, const nm_statics* st_extra, nm_particles* extra,
                         void* stream);

/* Particle-sharded substep (no reference counterpart - the reference is single-device).  Every rank
 * owns a fixed subset of the particles and a full grid handle; a grid node receives contributions from several ranks
 * only inside 4x4x4-node blocks that more than one rank touches.  The substep of mpm.py:279-297 / 299-319 is split
 * at the two points where those blocks have to be summed over the ranks, and the caller runs the collectives
 * (RCCL through torch.distributed) in between:
 *
 *   forward : nm_mpm_p2g                                     clear + scatter of the rank's particles (mpm.py:281-290)
 *             nm_mpm_active_list -> all-gather               the rank's touched-block list: out[0] = count, out[1..cap] = ids
 *             nm_mpm_shared_blocks                           blocks listed by >= 2 ranks, in an order all ranks agree on
 *             nm_mpm_blocks_pack(0) -> all-reduce(sum) -> nm_mpm_blocks_unpack(0)     {mv, m} of those blocks
 *             nm_mpm_forward_finish                          grid_op + g2p (mpm.py:291-297), writes the grid cache record
 *   backward: nm_mpm_backward_begin                          restore the grid from the record + scatter of the g2p adjoint
 *             nm_mpm_blocks_pack(1) -> all-reduce(sum) -> nm_mpm_blocks_unpack(1)     adjoint of the node velocities
 *             nm_mpm_backward_finish                         grid_op adjoint + p2g adjoint
 *
 * `shared` (device, int32[2 + 2*cap_shared], caller-owned, kept per substep for the backward): [0] number of shared
 * blocks, [1] status bits, [2..] block ids, [2+cap_shared..] 1 where this rank lists the block itself.  Status bits
 * (also OR-ed into *status, a device int32 the caller polls): 1 = some rank's list exceeded `cap`, 2 = more than
 * cap_shared shared blocks, 4 = the grid cache record overflowed (nm_mpm_forward_finish).  Any bit means the results
 * of that substep are incomplete: the caller must raise, enlarge the capacity and redo the roll-out.
 * pack writes cap_shared*64 float4 (zeros for blocks the rank does not list and for the unused tail), so the
 * all-reduce has a fixed size and needs no host synchronisation. */
int nm_mpm_p2g(nm_mpm* h, int32_t n, const nm_statics* st, const nm_particles* cur, void* stream);
int nm_mpm_active_list(nm_mpm* h, int32_t* out, int32_t cap, void* stream);
/* The same for the 27-neighbourhood (in blocks) of the rank's touched blocks: what the sharded roll-out announces once per
 * frame (nm_rollout_forward_sharded).  Exported so that the caller can size `cap` / `cap_shared` from a probe. */
int nm_mpm_dilated_list(nm_mpm* h, int32_t* out, int32_t cap, void* stream);
size_t nm_mpm_shared_workspace(int32_t world, int32_t cap);
int nm_mpm_shared_blocks(nm_mpm* h, const int32_t* gathered, int32_t world, int32_t cap, int32_t* shared,
                         int32_t cap_shared, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int nm_mpm_blocks_pack(nm_mpm* h, int32_t which, const int32_t* shared, int32_t cap_shared, float* buf, void* stream);
int nm_mpm_blocks_unpack(nm_mpm* h, int32_t which, const int32_t* shared, int32_t cap_shared, const float* buf,
                         void* stream);
int nm_mpm_forward_finish(nm_mpm* h, int32_t n, const nm_statics* st, const nm_particles* cur, nm_particles* next,
                          void* gridrec, int32_t cap_blocks, int32_t* status, void* stream);
int nm_mpm_backward_begin(nm_mpm* h, int32_t n, const nm_statics* st, const nm_particles* cur, const nm_particles* next,
                          const nm_particles* gnext, nm_particles* gcur, const void* gridrec, int32_t cap_blocks,
                          void* stream);
int nm_mpm_backward_finish(nm_mpm* h, int32_t n, const nm_statics* st, const nm_particles* cur, nm_particles* gcur,
                           void* stream);

/* Introspection for tests / roofline accounting: number of touched 4x4x4-node blocks and nodes with
 * mass > 0 after the last p2g.  Synchronises the stream. */
int nm_mpm_grid_stats(nm_mpm* h, int32_t* active_blocks, int32_t* nodes_with_mass, void* stream);
/* Copies the dense grid of the last forward (mv (G,G,G,3), m (G,G,G), v (G,G,G,3)) for tests. */
int nm_mpm_grid_export(nm_mpm* h, float* mv, float* m, float* v, void* stream);

/* Colliders (no reference counterpart: the reference's only obstacle is the box of mpm.py:373-429).  A collider is a rigid
 * shape in simulation coordinates (the unit cube; grid node (i,j,k) sits at (i,j,k) dx).  After the box boundary condition
 * every node with sdf < 0 has its velocity u replaced, collider by collider in list order; with v_c the collider's own
 * velocity, n its outward unit normal at the node, w = u - v_c and vn = w.n:
 *   sticky   : u' = v_c
 *   slip     : u' = u - vn n                                   if vn < 0, else u
 *   friction : u' = v_c + max(0, 1 + mu vn / |vt|) vt          if vn < 0 (vt = w - vn n; u' = v_c when vt = 0), else u
 * Shapes: half-space (solid where (p - center).normal < 0), sphere (radial normal; +x at the centre itself), oriented box
 * (rot: row-major, columns = the box axes in simulation coordinates; the normal at an inside node is the outward axis of the
 * face with the smallest penetration depth, ties to the lowest axis index).
 * Geometry is not differentiated; nm_mpm_backward* applies the transposed Jacobians du'/du in reverse list order, with the
 * colliders the handle holds at the time of the backward call.
 * Per-operator path only: nm_mpm_forward / _ex and nm_mpm_backward / _ex.  Every other entry point that steps the grid
 * (nm_mpm_forward_extra, the sharded substep calls, nm_rollout_*) returns NM_ERR_INVALID on a handle that holds colliders. */
#define NM_MAX_COLLIDERS 8
#define NM_COLLIDER_PLANE 0
#define NM_COLLIDER_SPHERE 1
#define NM_COLLIDER_BOX 2
#define NM_SURFACE_STICKY 0
#define NM_SURFACE_SLIP 1
#define NM_SURFACE_FRICTION 2
typedef struct nm_collider {
  int32_t shape;     /* NM_COLLIDER_* */
  int32_t surface;   /* NM_SURFACE_* */
  float friction;    /* Coulomb mu >= 0 (friction surface only) */
  float center[3];   /* plane: a point on it; sphere, box: the centre */
  float normal[3];   /* plane: unit outward normal */
  float radius;      /* sphere */
  float half[3];     /* box: half extents along its own axes */
  float rot[9];      /* box: rotation, row-major */
  float velocity[3]; /* v_c */
} nm_collider;
/* Host only: validates and copies `n` colliders into the handle (n = 0 removes them); no device work, no synchronisation,
 * may be called between any two substeps.  NM_ERR_INVALID, with a message that names the field: null handle, n outside
 * 0..NM_MAX_COLLIDERS, unknown shape / surface, a plane normal that is not unit within 1e-4, a non-positive radius / half
 * extent, a negative friction, a non-finite centre or velocity, a box rotation that is not orthonormal within 1e-4 or is a
 * reflection. */
int nm_mpm_set_colliders(nm_mpm* h, int32_t n, const nm_collider* host);

/* Field colliders (no reference counterpart; device functions: csrc/nm_collide_field.h; the same definition in fp64 torch:
 * neuma_amd/extras/colliders.py apply_field_collider): a rigid obstacle whose shape is a signed distance field phi (negative
 * inside) sampled on a regular lattice - node (ix, iy, iz) at origin + (ix, iy, iz) spacing in simulation coordinates, value
 * phi[(ix ny + iy) nz + iz] - e.g. the field of a closed triangle mesh (neuma_amd/mesh_sdf.py).  At the grid node at p:
 *   q = (p - origin) / spacing; the node is outside unless 0 <= q_a <= dims_a - 1 on all three axes (a NaN is outside);
 *   cell i_a = min(floor(q_a), dims_a - 2), fraction t = q - i;
 *   phi(p) = the trilinear interpolant of the cell's eight corner values: along z a_xy = f_xy0 + t_z (f_xy1 - f_xy0), along y
 *   b_x = a_x0 + t_y (a_x1 - a_x0), along x phi = b_0 + t_x (b_1 - b_0);
 *   the node is inside iff phi(p) < 0;
 *   the normal is n = g / |g|, g the analytic gradient of that same interpolant in t: g_x = b_1 - b_0, g_y = the x-interpolant
 *   of a_x1 - a_x0, g_z = the xy-interpolant of f_xy1 - f_xy0; n = +x where |g| = 0 (as the sphere at its centre).
 * Given n, the collider's own velocity v_c, its surface and mu, the response is exactly the sticky / slip / friction law of
 * the colliders above, and nm_mpm_backward* applies its transposed Jacobian du'/du; geometry is not differentiated.  Field
 * colliders are applied behind ALL analytic colliders, in list order, and their adjoints in reverse in front of the analytic
 * ones.  With none set no kernel is launched for them.  `origin` is the position of lattice node (0,0,0) NOW: a moving
 * collider is moved by the caller (origin += velocity dt, set again).  Every entry point that refuses a handle holding
 * colliders (above) refuses one holding field colliders, with the same message. */
#define NM_MAX_FIELD_COLLIDERS 4
typedef struct nm_field_collider {
  int32_t surface;   /* NM_SURFACE_* */
  float friction;    /* Coulomb mu >= 0 (friction surface only) */
  float velocity[3]; /* v_c */
  float origin[3];   /* simulation coordinates of lattice node (0,0,0), now */
  float spacing;     /* lattice spacing > 0 */
  int32_t dims[3];   /* nodes per axis, each >= 2, at most 2^27 in all */
  const float* phi;  /* DEVICE, prod(dims) floats; the caller keeps it alive while the handle holds the collider */
} nm_field_collider;
/* Host only, like nm_mpm_set_colliders: validates and copies `n` field colliders into the handle (n = 0 removes them); no device
 * work, no synchronisation.  NM_ERR_INVALID, with a message that names the field: null handle, n outside
 * 0..NM_MAX_FIELD_COLLIDERS, unknown surface, a negative friction, a non-finite origin or velocity, spacing <= 0, a dim < 2, more
 * than 2^27 nodes, a null phi.  A refused call leaves the set as it was. */
int nm_mpm_set_field_colliders(nm_mpm* h, int32_t n, const nm_field_collider* host);

/* Contact report (no reference counterpart; device code: csrc/nm_contact.h; the same definition in fp64 torch:
 * neuma_amd/extras/contact.py): the impulse the body hands to each obstacle in one substep.  With {mv, m} the grid of the
 * substep, at every node i with m_i > 0 at p_i = (i, j, k) dx:
 *   u^(0) = mv / (m + eps) + g dt                   (u_free)
 *   u^(1) = BC(u^(0))                               (the box boundary condition)
 *   u^(c+1) = collider c's response to u^(c)        (c = 1 .. R-1 in the order they are applied: analytic, then field colliders)
 * Row r (row 0: the box walls; row r >= 1: collider r) holds NM_CONTACT_COLS doubles:
 *   J[3]   sum_i m_i (u_i^(r) - u_i^(r+1))                    the linear impulse on the obstacle
 *   L[3]   sum_i m_i p_i x (u_i^(r) - u_i^(r+1))              the angular impulse about the simulation origin
 *   N      sum_i m_i (u_i^(r+1) - u_i^(r)) . n_i  over the nodes inside the collider, n_i its outward normal there: >= 0 for
 *          slip and friction, possibly negative (adhesion) for sticky; 0 in the walls row
 *   mass   sum m_i over the nodes with mass inside the collider (walls row: in the boundary layers, an index < bound or
 *          >= G - bound on any axis)
 *   nodes  the number of those nodes, as a double
 * Momentum: sum_i m_i u_free,i - sum_r J_r is the momentum g2p hands back to the particles.  Force and torque are left to the
 * caller: F = J / dt, torque about r0 = (L - r0 x J) / dt.  Units are simulation units: lengths of the unit cube, masses
 * rho * vol, no conversion to world units.
 * The velocities are evaluated in fp32 by the device functions the forward uses; differences, products and sums are fp64 in
 * the fixed order of csrc/nm_reduce.h (no atomics: two calls on the same handle state return identical bits).
 * Reads the grid the last nm_mpm_forward / _ex on this handle left, with the colliders the handle holds NOW: call it before
 * moving them.  Writes only `rows` and a workspace the handle owns (allocated on first use); the grid, the lists and the counters
 * are untouched.  Does not synchronise and reads nothing back.  With no colliders it writes the walls row alone.  NM_ERR_INVALID
 * with a message "contact: ..." for a null handle or null rows. */
#define NM_CONTACT_COLS 9
/* rows: DEVICE, (1 + analytic + field colliders) x 9 doubles: walls first, then the colliders in the order they are applied */
int nm_mpm_contact(nm_mpm* h, double* rows, void* stream);

/* Rigid bodies (no reference counterpart; device code: csrc/nm_rigid.h + the body variants of the collide / contact kernels; the
 * same definition in fp64: neuma_amd/extras/rigid.py; prose: DESIGN.md section 7 "Rigid bodies").  A rigid body b refers to one
 * analytic collider of the handle's list by index; it must be a sphere or a box (a plane is refused with a message naming the
 * entry; field colliders are not in that list at all).  nm_collider keeps its layout.
 * Constants: mass M > 0; body-frame principal inertia I_b[3] > 0 (sphere: 2/5 M r^2; box with half extents h:
 *   M/3 (h_y^2 + h_z^2, h_x^2 + h_z^2, h_x^2 + h_y^2); the caller fills them); flags NM_RIGID_NO_GRAVITY (gravity is on by default
 *   and is the handle's) and NM_RIGID_KINEMATIC (impulses and gravity are ignored and the body keeps v and w: a paddle, a stirrer).
 * State, fp64, owned by the handle, on the device: centre c[3], unit quaternion q[4] (wxyz; for a box R(q) replaces `rot`),
 *   linear momentum P[3], angular momentum Lc[3] about the centre in simulation axes.  Initialised from the collider's `center`,
 *   `rot` (through its quaternion), `velocity` (P = M v) and `angular_velocity` (Lc = R diag(I_b) R^T w).  Derived:
 *   v = P / M, w = R diag(1 / I_b) R^T Lc (a kinematic body: the `angular_velocity` it was given; its Lc is never touched).
 * Response: at the grid node at p the collider's own velocity is v_c(p) = v + w x (p - c), evaluated in fp32 from the fp32 copies
 *   of c, v, w (three more roundings per component than a prescribed collider's constant); nothing else of the sticky / slip /
 *   friction law changes, and a box's geometry uses the fp32 copy of R(q).
 * Step (nm_mpm_rigid_step; call it where a prescribed collider would be moved, after the forward and after any nm_mpm_contact):
 *   reads the grid the last nm_mpm_forward / _ex left, with the poses that forward collided against, takes every body's contact
 *   row J, L (about the origin) by the launches and the fixed-order fp64 reduction of nm_mpm_contact - which, called between the
 *   forward and the step, returns the very rows the step consumes -, and in one small kernel (one wave, one lane per body, fp64)
 *     P  += J + M g dt                                  (g, dt: the handle's fp32 values, widened)
 *     Lc += L - c x J                                   (the old c)
 *     c  += (P / M) dt
 *     q  <- normalize(exp(w dt / 2) (x) q)              the new w with R of the old q; the exact exponential
 *                                                       (cos(theta/2), sin(theta/2) w / |w|), theta = |w| dt, with
 *                                                       sin(theta/2)/theta = 1/2 - theta^2/48 + theta^4/3840 for theta < 1e-2
 *   then refreshes the fp32 pose the collide kernels read.  Nothing is read back, nothing happens on the host.
 * A handle without bodies launches the kernels it launched before, with the arguments it passed before (their device code is the
 *   code it was); one with bodies launches k_grid_collide_rigid / k_contact_rows_rigid, whose body entries read c, R, v, w from a
 *   small wave-uniform device record.  k_contact_rows_rigid visits the active blocks by block id (over the epoch flags), not in the
 *   order of the active-block list, which differs from run to run: with bodies, nm_mpm_contact's rows - and with them the bodies'
 *   states - are the same bits in two runs whose grids are.
 * nm_mpm_grid_export on a handle with bodies collides the blocks no particle touched at the pose the device record holds NOW, while
 *   the touched blocks hold the velocities the forward collided: the export is consistent between the forward and the step only (a
 *   prescribed mover has the same property once the caller has moved it).
 * Forward only: nm_mpm_backward / _ex return NM_ERR_INVALID ("rigid bodies: forward only") on a handle that holds bodies; every
 *   entry point that refuses colliders refuses bodies with them (a body is a collider).
 * Out of scope: body-body contact; contact between a body and the box walls or any other collider (a body is moved by the material
 *   and gravity alone and may leave the cube); mesh colliders as bodies; differentiation.
 * Stability (documented, not enforced): the coupling is explicit.  For a sticky body the velocity change per substep is
 *   (sum m_i / M)(u_mean - v), sum m_i the `mass` column of its contact row: it overshoots beyond a ratio of 1 and diverges beyond 2.
 * nm_mpm_set_colliders on a handle that holds bodies: a list of the SAME length keeps them - the `center`, `rot` and `velocity` of
 *   a body's entry are ignored (the device record has them), its shape must stay a sphere or a box, its radius / half / surface are
 *   taken; a list of another length removes the bodies. */
#define NM_RIGID_KINEMATIC 1
#define NM_RIGID_NO_GRAVITY 2
#define NM_RIGID_STATE_COLS 19
typedef struct nm_rigid_body {
  int32_t collider;             /* index into the analytic colliders the handle holds now */
  int32_t flags;                /* NM_RIGID_* */
  double mass;                  /* M > 0 */
  double inertia[3];            /* I_b > 0, body frame */
  double angular_velocity[3];   /* initial w, simulation axes */
} nm_rigid_body;
/* Validates and installs `n` bodies (n = 0 removes them), builds their initial state on the host in fp64 and uploads it; it
 * synchronises the device (a set-up call).  NM_ERR_INVALID with a message "rigid body <q>: <field>: ..." naming the field: a
 * collider index out of range, an entry that is a plane, the same entry twice (duplicate), unknown flag bits, a non-positive or
 * non-finite mass or inertia, a non-finite angular_velocity; "rigid bodies: ..." for a null handle / array or n out of range.  A
 * refused call leaves the handle as it was. */
int nm_mpm_set_rigid_bodies(nm_mpm* h, int32_t n, const nm_rigid_body* host);
int32_t nm_mpm_num_rigid_bodies(const nm_mpm* h);
/* One substep of every body (above).  Asynchronous on `stream`; a no-op on a handle without bodies. */
int nm_mpm_rigid_step(nm_mpm* h, void* stream);
/* rows: DEVICE, (1 + analytic + field colliders) x NM_CONTACT_COLS doubles: a copy of the contact rows the last nm_mpm_rigid_step
 * consumed (nm_mpm_contact's layout; undefined before the first step).  Asynchronous on `stream`; a no-op without bodies. */
int nm_mpm_rigid_rows(nm_mpm* h, double* rows, void* stream);
/* out: DEVICE or pinned host memory, n x NM_RIGID_STATE_COLS doubles per body in the order they were set: c[3], q[4], P[3],
 * Lc[3], v[3], w[3].  Asynchronous on `stream`; a no-op on a handle without bodies. */
int nm_mpm_rigid_state(nm_mpm* h, double* out, void* stream);

/* Drawing colliders (no reference counterpart; kernels: csrc/nm_draw.hip + csrc/nm_collide_ray.h; the same definition in fp64:
 * neuma_amd/extras/collider_draw.py; prose: DESIGN.md section 7).  Three calls in front of and behind unchanged
 * nm_raster_forward_ex renders; nothing here is differentiated.
 * Coordinates: colliders live in simulation coordinates, renders in render coordinates, p_r = a * p_s + b per axis (map_a,
 *   map_b: 3 host floats each, a > 0).  Rays are cast in simulation space from o_s = (o_r - b) / a with the UN-normalised
 *   direction d_s = d_r / a (d_r a unit vector), so the ray parameter t is the render-space distance for any a > 0; a
 *   render-space normal is normalize(n_s / a).
 * Drawn solid of a collider: its shape cut by the unit cube [0,1]^3 (the only region where it acts on the grid; a half-space
 *   gets a finite body).  Both are convex: the ray is inside for t in (t_in, t_out), t_in the largest entry and t_out the
 *   smallest exit over the constraints - the half-space's inequality / the sphere's quadratic / the box's three slabs in its
 *   own frame, then the cube's three slabs.  The normal at t_in is that of the constraint that gave it (of equal entries the
 *   first in the order shape, cube x, y, z).  Hit: t_in < t_out and t_out > 0, at t = max(t_in, 0); t_in < 0 means the
 *   origin is inside: t = 0 and the normal faces the camera.
 * Pixel ray: origin cfg->campos; direction through the point that cfg's projmatrix maps to the pixel's centre, ndc
 *   ((2 px + 1) / W - 1, (2 py + 1) / H - 1), on the far plane (ndc z = 1): with inv_proj = projmatrix^-1 (16 host doubles,
 *   row-major, row-vector convention hom = clip inv_proj; the caller inverts in fp64) the direction is
 *   hom.xyz - hom.w campos for clip = (x, y, 1, 1), folded in fp64 on the host.  The nearest hit over the colliders wins
 *   (of equal t the first in list order).
 * Shade: rgb = color * k * (0.35 + 0.65 max(0, n_r.l)), l = -d_r (the unit vector from the hit to the camera: a headlight).
 *   k = 0.8 on the odd cells, floor(cu) + floor(cv) odd, of a checkerboard on a plane's own face when its style has
 *   checker > 0: (cu, cv) = ((p_s - center).u, (p_s - center).v) / checker with the frame e = the coordinate axis along which
 *   |normal| is smallest (the lowest of equal ones), u = normalize(normal x e), v = normal x u; k = 1 everywhere else (cube
 *   faces, spheres, boxes, camera inside).
 * Occlusion is per Gaussian, not per pixel: a Gaussian is hidden when the segment o_s + u (mean_s - o_s), u in (0, 1), meets a
 *   drawn solid before u = 1 or the mean lies inside one: u_in < u_out, u_out > 0 and u_in < 1.  It is shown or dropped as a
 *   whole by its centre.
 * Frame: besides img_all (the usual render over the configured background) the caller renders, with opacity_front and bg = 0,
 *   rgb_front (the frame's colours) and a_front (channel 0 of a colors_precomp = 1 render); then out = rgb_front +
 *   (1 - a_front) shade where hit >= 0 and out = img_all, bit for bit, elsewhere. */
struct nm_raster_cfg; /* the rasterizer's per-view settings, below */
typedef struct nm_collider_style {
  float color[3]; /* rgb in 0..1 */
  float checker;  /* planes: checkerboard cell size in simulation units, 0 = plain; ignored for spheres and boxes */
} nm_collider_style;
/* t (H,W; +inf where nothing is hit), shade (3,H,W; 0 there), hit (H,W int32: collider index or -1) for the whole image of
 * cfg (image_height, image_width, campos are read).  n = 0 is valid.  NM_ERR_INVALID, naming the field: null pointers, n outside
 * 0..NM_MAX_COLLIDERS, a <= 0 (map_a), non-finite style values / map / camera / inv_proj, and nm_mpm_set_colliders' geometry
 * checks (shape, center, normal, radius, half, rot). */
int nm_collider_cast(const struct nm_raster_cfg* cfg, const double* inv_proj, const float* map_a, const float* map_b, int32_t n,
                     const nm_collider* colliders, const nm_collider_style* styles, float* t, float* shade, int32_t* hit,
                     void* stream);
/* opacity_front (K,1) = 0 where the Gaussian at means3D (K,3; render coordinates) is hidden from campos (3 host floats, render
 * coordinates), opacity (K,1) elsewhere; hidden (K uint8, may be NULL) = the flags.  Same validation. */
int nm_collider_hide(const float* campos, const float* map_a, const float* map_b, int32_t n, const nm_collider* colliders,
                     int32_t k, const float* means3D, const float* opacity, float* opacity_front, uint8_t* hidden, void* stream);
/* out (3,H,W) from img_all, rgb_front, shade (3,H,W), a_front (H,W: channel 0 of the alpha render) and hit (H,W).  Writes the
 * pixel rows of cfg's stripe [16 tile_y0, 16 tile_y1) only (every row when tile_y1 <= tile_y0). */
int nm_collider_compose(const struct nm_raster_cfg* cfg, const float* img_all, const float* rgb_front, const float* a_front,
                        const float* shade, const int32_t* hit, float* out, void* stream);

/* Drawing mesh colliders (no reference counterpart; kernels: k_field_cast / k_field_hide in csrc/nm_draw.hip, the trace:
 * csrc/nm_field_ray.h; the same definition in fp64: neuma_amd/extras/mesh_draw.py; prose: DESIGN.md section 7).  Two IN-OUT passes
 * behind nm_collider_cast / nm_collider_hide; nm_collider_compose needs only hit >= 0 and stays as it is.
 * Drawn solid of a field collider: the zero level set's inside, {phi < 0}, of the trilinearly interpolated phi ("Field colliders"
 *   above), cut by the lattice box [origin, origin + (dims - 1) spacing] and by the unit cube - the solid the simulator collides
 *   with, at the lattice's resolution; `origin` is where the collider is NOW.
 * Rays: exactly those of "Drawing colliders": o_s = (o_r - b) / a, the un-normalised d_s = d_r / a (t is the render-space
 *   distance), L = |d_s|.
 * Interval: [t0, t1] = t >= 0, the three slabs of the unit cube, the three slabs of the lattice box; t0 is the largest entry
 *   (of equal entries the first in the order t >= 0, cube x, y, z, lattice x, y, z), t1 the smallest exit.  With t_end =
 *   min(t1, the t already in the buffer): t0 >= t_end is a miss.
 * Sample: phi(t) is the interpolant at o_s + t d_s, q = (p - origin) / spacing, cell i_a = max(min(floor(q_a), dims_a - 2), 0)
 *   (a point a rounding error outside the lattice extrapolates its border cell), fraction q - i.
 * Face hit: phi(t0) < 0: the hit is at t0 and the normal is that of the slab that gave t0; t0 = 0 (the camera is inside the
 *   solid): the normal faces the camera, n_r.l = 1.
 * March: tau = 1e-3 spacing; at most 192 times: phi(t) <= tau -> converged; otherwise t += max(phi, tau) / L, and t >= t_end is
 *   a miss.  A ray still marching after 192 steps is a miss.  (Step factor 1: phi is a distance in simulation units.)
 * Polish: three Newton steps along the ray, t -= phi / (grad . d_s) with the analytic gradient of the interpolant in simulation
 *   units (divided by spacing) in the cell that holds the point, each taken only while grad . d_s < 0; t is kept in [t0, t1].
 * Normal and shade: n_s = grad / |grad| at the final t (+x where the gradient vanishes), n_r = normalize(n_s / a), rgb = color *
 *   (0.35 + 0.65 max(0, n_r . -d_r)); a style's checker is ignored.
 * Merge: a field hit replaces a pixel only where its final t is strictly smaller than the t in the buffer - analytic colliders win
 *   ties, and among fields the first in list order; hit becomes hit_base + j (the caller passes the number of analytic colliders).
 *   A pixel no field changes is not written.
 * Occlusion per Gaussian: the same interval, face hit and march on the segment o_s + u (mean_s - o_s) with t_end = min(t1, 1) (no
 *   polish); a Gaussian is hidden when that hits, or when the mean lies in the unit cube and inside the field ("Field colliders":
 *   on the lattice and phi(mean) < 0).  Hidden Gaussians get opacity_front = 0 and hidden = 1; the others are not written. */
/* t, shade, hit: what nm_collider_cast has written (n = 0 there is valid and writes +inf / 0 / -1), updated in place.  n = 0 is a
 * valid no-op.  NM_ERR_INVALID, naming the field: the map, style, camera and inv_proj checks of nm_collider_cast, n outside
 * 0..NM_MAX_FIELD_COLLIDERS, a negative hit_base, and nm_mpm_set_field_colliders' checks (surface, friction, velocity, origin,
 * spacing, dims, phi) as "field collider <j>: <field>: ...". */
int nm_collider_cast_field(const struct nm_raster_cfg* cfg, const double* inv_proj, const float* map_a, const float* map_b, int32_t n,
                           const nm_field_collider* fields, const nm_collider_style* styles, int32_t hit_base, float* t, float* shade,
                           int32_t* hit, void* stream);
/* opacity_front (K,1) and hidden (K uint8, may be NULL): what nm_collider_hide has written, updated in place.  Same validation. */
int nm_collider_hide_field(const float* campos, const float* map_a, const float* map_b, int32_t n, const nm_field_collider* fields,
                           int32_t k, const float* means3D, float* opacity_front, uint8_t* hidden, void* stream);

/* ------------------------------------------------------------------ SVD (modules/nclaw/warp/svd.py) */

/* SVDFunction.forward / batch_svd, svd.py:12-38, 61-96.  F (N,3,3) -> U (N,3,3), sigma (N,3), Vh (N,3,3);
 * U, V in SO(3), sigma0 >= sigma1 >= |sigma2|, sign(sigma2) = sign(det F). */
int nm_svd3_fwd(int32_t n, const float* F, float* U, float* sigma, float* Vh, void* stream);
/* SVDFunction.backward, svd.py:41-57 (adjoint of wp.svd3 with the 1e-6 denominator clamp). */
int nm_svd3_bwd(int32_t n, const float* U, const float* sigma, const float* Vh, const float* gU,
                const float* gsigma, const float* gVh, float* gF, void* stream);

/* ------------------------------------------------------------------ constitutive nets (modules/nclaw/material/meta.py) */

/* Effective (LoRA-merged, loralib.py:209-213) weights, row-major, no bias (meta.py:20-42):
 * w0 (64,13), w1 (64,64), w2 (9,64). */
typedef struct nm_mlp {
  const float* w0;
  const float* w1;
  const float* w2;
} nm_mlp;

#define NM_ELASTICITY 0 /* InvariantFullMetaElasticity.forward, meta.py:196-221: out = R sym(X) F^T */
#define NM_PLASTICITY 1 /* InvariantFullMetaPlasticity.forward, meta.py:468-489: out = F + alpha R sym(X) */

int nm_material_fwd(int32_t n, int32_t kind, float alpha, const float* F, const nm_mlp* w,
                    float* out, void* stream);
/* Backward: gF (N,3,3) overwritten; gw0/gw1/gw2 (same shapes as the weights) overwritten with the
 * sum over particles (may be NULL to skip weight gradients).  workspace: device scratch of at
 * least nm_material_bwd_workspace(n) bytes. */
size_t nm_material_bwd_workspace(int32_t n);
int nm_material_bwd(int32_t n, int32_t kind, float alpha, const float* F, const nm_mlp* w,
                    const float* gout, float* gF, float* gw0, float* gw1, float* gw2,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Same with flags: NM_BWD_ACCUMULATE adds into gw0/gw1/gw2 instead of overwriting (BPTT over substeps);
 * NM_BWD_POLAR_ADJOINT replaces the reference's SVD adjoint - warp's adj_svd3 behind warp/svd.py:41-57, whose denominators
 * 1/(s_j^2 - s_i^2) are clamped at 1e-6 and which therefore returns ~0 for the rotation path where two singular values
 * coincide (F = I) - by the exact derivative of the polar rotation.  nm_material_bwd == flags 0 == the reference's gradient. */
#define NM_BWD_ACCUMULATE 1
#define NM_BWD_POLAR_ADJOINT 2
int nm_material_bwd_ex(int32_t n, int32_t kind, float alpha, const float* F, const nm_mlp* w,
                       const float* gout, float* gF, float* gw0, float* gw1, float* gw2,
                       int32_t flags, void* workspace, size_t workspace_bytes, void* stream);

/* LinearLoRA merge, modules/nclaw/material/loralib.py:209-213: Weff (out,in) = W + scaling * B (out,r) @ A (r,in), and its
 * adjoint gB = scaling * gW A^T, gA = scaling * B^T gW (what autograd derives from loralib.py:216-224). */
int nm_lora_merge(int32_t out_f, int32_t in_f, int32_t r, float scaling, const float* W, const float* B,
                  const float* A, float* Weff, void* stream);
int nm_lora_merge_bwd(int32_t out_f, int32_t in_f, int32_t r, float scaling, const float* gW, const float* B,
                      const float* A, float* gB, float* gA, void* stream);

/* The same for up to NM_LORA_MAX_LAYERS layers in ONE launch each way (a constitutive net has three, a frame merges both nets' six; per-layer launches
 * of these tiny matrices are pure launch latency).  merge: o0 = W + scaling * B A.  merge_bwd: W holds dL/dW_eff,
 * o0 = dL/dB, o1 = dL/dA. */
#define NM_LORA_MAX_LAYERS 8
typedef struct nm_lora_layer {
  int32_t out_f, in_f, r;
  float scaling;
  const float* W;
  const float* B;
  const float* A;
  float* o0;
  float* o1;
} nm_lora_layer;
int nm_lora_merge_layers(int32_t n, const nm_lora_layer* layers, void* stream);
int nm_lora_merge_layers_bwd(int32_t n, const nm_lora_layer* layers, void* stream);

/* ------------------------------------------------------------------ fused roll-out (experiments/finetune.py:360-364) */

/* S substeps of   stress = E(F); (x,v,C,F) = sim(x,v,C,F,stress); F = P(F)   (finetune.py:362-364,
 * render.py:305-309) enqueued natively, so the host pays one call per video frame instead of three
 * autograd nodes per substep.  `states` is a caller-owned checkpoint buffer of (S+1) records; record t
 * holds x (N,3) | v (N,3) | C (N,9) | F (N,9) | stress (N,9) contiguously (33*N floats; stress = E(F) of that
 * record, written by the forward pass for t < S).  The caller fills x,v,C,F of record 0; records 1..S are
 * written.  Nothing else is kept: the backward pass recomputes the trial F, the grid and all MLP activations
 * from the checkpoints (132 B/particle/substep instead of the reference's ~3.5 KB). */
typedef struct nm_rollout_cfg {
  int32_t substeps;
  float plasticity_alpha;
  int32_t grid_cache_blocks; /* capacity (in 4x4x4-node blocks) of each substep's grid cache record; 0 = no cache */
  int32_t cache_verified;    /* backward only: the caller has read nm_rollout_cache_status and every record is valid, so the
                              * (early-exit) fallback launches of p2g / grid_op can be left out altogether */
  int32_t svd_adjoint;       /* backward only: NM_SVD_ADJOINT_REFERENCE (0, clamped like warp's adj_svd3) or NM_SVD_ADJOINT_POLAR */
  void* svd_cache;           /* optional device buffer of nm_rollout_svdcache_bytes(n, substeps): the forward pass keeps U, sigma, V of
                              * both nets' inputs of every substep (168 B/particle/substep) and the reverse sweep reads them back
                              * instead of repeating the Jacobi SVD; NULL = recompute (same results to rounding: the trial F the
                              * reverse sweep rebuilds from the checkpoints differs from the forward's in the last bit) */
  void* act_cache;           /* optional device buffer of nm_rollout_actcache_bytes(n, substeps): the forward pass keeps what the
                              * reverse sweep cannot cheaply rebuild - the second hidden layer's activations and GELU derivatives
                              * and the output of both nets, 1.2 KB/particle/substep - and the reverse sweep loads it, recomputing
                              * only the first layer (16 of the forward pass's 96 matrix instructions per tile); NULL = recompute
                              * everything.  Same arithmetic, same results. */
  int32_t weights_prepared;  /* nm_rollout_backward only: the workspace is the one the forward call of this node used and
                              * nothing has touched it since, so both nets' weights still sit there in operand order and the
                              * reverse sweep skips that launch.  0 (and every caller that does not know) = prepare them. */
  int32_t last_gF_zero;      /* (not the sharded forms) backward: the caller promises that dL/dF of the last record
                              * (gstate_last + 15 n) is zero everywhere - a loss that sees the final positions only, as the
                              * reference's does (the covariance push-forward is not differentiated, tune/utils.py:353-373).  The
                              * last substep's plasticity adjoint then has nothing to propagate (zero dL/dF, zero weight
                              * gradients) and is not launched.  Given to nm_rollout_forward as well, the last plasticity step
                              * leaves no SVD / activation records (nobody would read them); nm_rollout_backward WITHOUT the flag over
                              * caches whose forward sweep ran with it fails with NM_ERR_INVALID.  The sharded pair ignores the
                              * word (its forward sweep always writes the records) but keeps the same books: its reverse sweep
                              * refuses caches last written by such a forward sweep too.  0 = make no assumption. */
} nm_rollout_cfg;
#define NM_SVD_ADJOINT_REFERENCE 0
#define NM_SVD_ADJOINT_POLAR 1
size_t nm_rollout_workspace(int32_t n, int32_t substeps);
size_t nm_rollout_svdcache_bytes(int32_t n, int32_t substeps);
size_t nm_rollout_actcache_bytes(int32_t n, int32_t substeps);
/* bytes of the optional `gridcache` buffer: substeps records of nm_mpm_gridcache_bytes(grid_cache_blocks) */
size_t nm_rollout_gridcache_bytes(int32_t substeps, int32_t grid_cache_blocks);
/* Asynchronous read-back of the S record headers of a grid cache into host memory (pinned recommended): status[t] = number
 * of cached blocks of substep t, or -1 if that substep outgrew the capacity.  Valid once the stream has passed this point. */
int nm_rollout_cache_status(const void* gridcache, const nm_rollout_cfg* cfg, int32_t* status_host, void* stream);
/* gridcache (may be NULL): written by the forward pass, handed unchanged to nm_rollout_backward, which then restores
 * each substep's grid instead of recomputing p2g (see nm_mpm_forward_ex). */
int nm_rollout_forward(nm_mpm* h, int32_t n, const nm_rollout_cfg* cfg, const nm_statics* st,
                       const nm_mlp* elasticity, const nm_mlp* plasticity, float* states, void* gridcache,
                       void* workspace, size_t workspace_bytes, void* stream);
/* Forward sweep layout (process-wide, default on): plasticity of substep t and elasticity of substep t+1 - the two calls
 * experiments/finetune.py:364 and :362 make back to back across the loop edge - run as ONE launch per substep boundary, F_{t+1}
 * passing from one net to the other in registers; off = one launch per net.  Results are bit-identical either way. */
int nm_rollout_set_forward_pair(int32_t on);
/* gstate_last: dL/d(x,v,C,F of record S) (24*N floats: x|v|C|F); gstate_first: dL/d(x,v,C,F of record 0) (written);
 * gw_e / gw_p: 5504 floats each = dL/d(w0 | w1 | w2) of the elasticity / plasticity nets, summed over
 * particles and substeps (overwritten). */
int nm_rollout_backward(nm_mpm* h, int32_t n, const nm_rollout_cfg* cfg, const nm_statics* st,
                        const nm_mlp* elasticity, const nm_mlp* plasticity, const float* states,
                        const void* gridcache, const float* gstate_last, float* gstate_first, float* gw_e,
                        float* gw_p, void* workspace, size_t workspace_bytes, void* stream);

/* Particle-sharded roll-out (no reference counterpart - the reference is single-device): the same S-substep
 * node for ONE rank's share of the particles.  The MPM part of every substep is cut at the two points where the grid
 * blocks that several ranks touch have to be summed ("Particle-sharded substep" above); the loop over substeps and phases
 * - launches and collectives alike - runs inside the library, on `stream`.  The collectives themselves are the caller's
 * (one process per GPU: torch.distributed over RCCL; any transport in tests): nm_comm is a table of two functions that
 * must enqueue, in stream order on `stream`,
 *   all_gather_i32      recv[r * count + i] = rank r's send[i]   (count = 1 + cap int32 per rank: the ranks' block lists)
 *   all_reduce_sum_f32  buf[i] = sum over ranks of buf[i]        (count = cap_shared * 256 floats: the shared blocks)
 * and return 0 on success.  send / recv / buf point into `shard_ws`.  Per roll-out: one all-gather (the ranks' block
 * neighbourhoods, negotiated at the first substep) and one 8-float all-reduce (the status bits, OR-ed over the ranks); per
 * substep: one all-reduce of the exchange buffer in the forward pass and one in the reverse sweep - or, with
 * exchange_peers_f32 and a peer set, one swap of the buffer with the neighbour ranks each.  gridcache is mandatory (grid_cache_blocks >= the blocks a rank
 * touches): the reverse sweep restores the already-summed grid from it - there is no recompute across ranks.
 * shard_ws: device memory of nm_rollout_shard_workspace(world, cap, cap_shared, substeps) bytes, written by the forward
 * pass (the shared-block list of every substep) and handed unchanged to the backward pass.  Capacity overflows do not
 * stop the roll-out: they set bits in a status word (nm_rollout_shard_status: 1 = a rank listed more than `cap` blocks,
 * 2 = more than `cap_shared` blocks are shared, 4 = a grid cache record overflowed, 8 = a particle left the neighbourhood its
 * rank announced, 16 = a block is shared with a rank outside nm_comm.peers) - any bit means the results are
 * incomplete and the caller must enlarge the capacity and redo the roll-out.  A rank with n = 0 particles takes part. */
typedef struct nm_comm {
  int32_t world, rank;
  int (*all_gather_i32)(void* user, const int32_t* send, int32_t* recv, int64_t count, void* stream);
  int (*all_reduce_sum_f32)(void* user, float* buf, int64_t count, void* stream);
  void* user;
  /* Optional neighbour-only exchange of the shared blocks (round 5).  A grid block is shared by the 2-3 ranks whose particle
   * ranges meet there, not by the world: instead of all-reducing the exchange buffer over every rank, a rank sends its buffer
   * to the ranks it shares at least one block with (`peers`, bit q = rank q; symmetric; sim/shard.py derives it from the same
   * all-gathered neighbourhood lists on every rank) and adds what they send, in ascending rank order - the same operands
   * in the same order on every owner of a block, so the owners still hold identical sums.
   *   exchange_peers_f32  send `count` floats at `send` to every rank in `peers` and receive that rank's `count` floats into
   *                       recv + k * count, k = the rank's position among the set bits of `peers` (ascending); stream-ordered.
   * NULL or peers == 0xFFFFFFFF: the all-reduce above.  A rank that turns out to share a block with a rank outside `peers`
   * sets status bit 16 (rank-uniform like the others): the caller re-derives `peers` and redoes the roll-out. */
  int (*exchange_peers_f32)(void* user, const float* send, float* recv, int64_t count, uint32_t peers, void* stream);
  uint32_t peers;
} nm_comm;
#define NM_COMM_ALL_RANKS 0xFFFFFFFFu
size_t nm_rollout_shard_workspace(int32_t world, int32_t cap, int32_t cap_shared, int32_t substeps);
int nm_rollout_forward_sharded(nm_mpm* h, int32_t n, const nm_rollout_cfg* cfg, const nm_statics* st,
                               const nm_mlp* elasticity, const nm_mlp* plasticity, float* states, void* gridcache,
                               void* workspace, size_t workspace_bytes, const nm_comm* comm, int32_t cap,
                               int32_t cap_shared, void* shard_ws, size_t shard_ws_bytes, void* stream);
int nm_rollout_backward_sharded(nm_mpm* h, int32_t n, const nm_rollout_cfg* cfg, const nm_statics* st,
                                const nm_mlp* elasticity, const nm_mlp* plasticity, const float* states,
                                const void* gridcache, const float* gstate_last, float* gstate_first, float* gw_e,
                                float* gw_p, void* workspace, size_t workspace_bytes, const nm_comm* comm, int32_t cap,
                                int32_t cap_shared, const void* shard_ws, size_t shard_ws_bytes, void* stream);
int nm_rollout_shard_status(const void* shard_ws, int32_t* status_host, void* stream);

/* Library-owned RCCL communicator (round 4; no reference counterpart - the reference is single-device).
 * With it the sharded roll-out's collectives are issued by the library itself, on the caller's stream, from the loop in
 * nm_rollout_forward_sharded / nm_rollout_backward_sharded: nm_rccl_comm fills an nm_comm whose two functions call
 * ncclAllGather / ncclAllReduce.  librccl is looked up with dlopen on first use (the copy already in the process - torch's -
 * first, then librccl.so.1): no link-time dependency; without RCCL these calls return NM_ERR_INVALID.
 *   nm_rccl_unique_id   rank 0 fills 128 bytes (ncclUniqueId) and hands them to the other ranks by any means
 *                       (neuma_amd/sim/shard.py: one torch.distributed broadcast)
 *   nm_rccl_create      collective over the group: ncclCommInitRank on the current HIP device
 *   nm_rccl_time_all_reduce  mean microseconds of `reps` in-place all-reduces of `count` floats (after `warm` untimed ones):
 *                       the start-up calibration of the shard cost model; collective, synchronises the stream
 *   nm_rccl_library     which librccl was bound ("" if none) */
typedef struct nm_rccl nm_rccl;
const char* nm_rccl_library(void);
int nm_rccl_unique_id(void* id128);
int nm_rccl_create(const void* id128, int32_t world, int32_t rank, nm_rccl** out);
int nm_rccl_destroy(nm_rccl* c);
int nm_rccl_comm(nm_rccl* c, nm_comm* out);
int nm_rccl_all_reduce_sum_f32(nm_rccl* c, float* buf, int64_t count, void* stream);
int nm_rccl_all_gather_i32(nm_rccl* c, const int32_t* send, int32_t* recv, int64_t count, void* stream);
/* nm_comm.exchange_peers_f32 on this communicator: ncclSend / ncclRecv to and from every rank in `peers` inside ONE group call */
int nm_rccl_exchange_peers_f32(nm_rccl* c, const float* send, float* recv, int64_t count, uint32_t peers, void* stream);
/* start-up calibration (like nm_rccl_time_all_reduce): mean microseconds of `reps` such exchanges of `count` floats */
int nm_rccl_time_exchange_peers(nm_rccl* c, const float* send, float* recv, int64_t count, uint32_t peers, int32_t warm, int32_t reps,
                                float* us_out, void* stream);
/* Which ranks share a block with this one: adj[q] = 1 iff a block of rank q's list in `gathered` (world x (1 + cap), the
 * all-gathered neighbourhood lists of nm_mpm_dilated_list) lies in THIS rank's current neighbourhood (device array of `world`
 * int32, adj[rank] = 0).  The predicate is symmetric, so the masks the ranks derive from it match pairwise. */
int nm_mpm_peer_ranks(nm_mpm* h, const int32_t* gathered, int32_t world, int32_t cap, int32_t rank, int32_t* adj, void* stream);
int nm_rccl_time_all_reduce(nm_rccl* c, float* buf, int64_t count, int32_t warm, int32_t reps, float* us_out, void* stream);

/* ------------------------------------------------------------------ Particle-GS binding (modules/tune/utils.py) */

/* torch.sparse.mm(bindings, X) of compute_bindings_xyz / compute_bindings_F, tune/utils.py:424-472,
 * on a CSR copy of the COO binding matrix: out[r,:] = sum_j val[j] * in[col[j],:], D columns.
 * The backward (B^T g) is the same call on the transposed CSR. */
int nm_spmm_csr(int32_t rows, int32_t D, const int32_t* rowptr, const int32_t* col,
                const float* val, const float* in, float* out, void* stream);
/* The reverse sweep's form of the same product (d loss / d particle positions, the adjoint of compute_bindings_xyz,
 * tune/utils.py:424-448, through finetune.py:373's (x - center) / size): out (rows x 3) = scale * A (in0 + in1 + in2 + in3),
 * the inputs being the views' dL/dmeans3D (in1..in3 may be NULL, in order), A the transposed CSR. */
int nm_spmm_csr_sum3(int32_t rows, const int32_t* rowptr, const int32_t* col, const float* val, const float* in0,
                     const float* in1, const float* in2, const float* in3, float scale, float* out, void* stream);
/* Binding construction (data preparation): gaussian_binding_with_clip_v1 / gaussian_binding,
 * modules/d3gs/utils/binding_utils.py:199-285 / 123-196.  Particle j binds to Gaussian k iff (x_j - mean_k)^T inv(cov_k)
 * (x_j - mean_k) <= threshold (= chi2.ppf(confidence, 3)); at most max_particles (<= 16) per Gaussian, the ones with the
 * smallest distance.  The particles are binned into the uniform grid (origin, cell edge, dims) the caller chooses; a
 * Gaussian only visits the cells under its ellipsoid's bounding box.  Outputs (caller-allocated): counts (K) = kept per
 * Gaussian, n_inside (K, may be NULL) = qualifying before the clip, cols (K x max_particles, ascending, -1 padded),
 * pvals (same shape, may be NULL) = their Mahalanobis distances.  Every kept particle has weight 1/counts[k]
 * (softmax of -ones, binding_utils.py:259-269).  No dense K x N matrix is ever formed. */
size_t nm_bind_build_workspace(int32_t n_particles, int32_t ncells);
int nm_bind_build(int32_t K, int32_t N, const float* means, const float* cov6, const float* particles,
                  const float* grid_origin, float cell, const int32_t* grid_dims, float threshold,
                  int32_t max_particles, int32_t* counts, int32_t* n_inside, int32_t* cols, float* pvals,
                  void* workspace, size_t workspace_bytes, void* stream);

/* deform_cov_by_F, modules/d3gs/utils/simulation_utils.py:25-48. */
int nm_cov_deform(int32_t k, const float* cov6, const float* F, float* out_cov6, void* stream);
/* Fused per-frame binding: means3D = k_prev + B (p_cur - p_prev);  F_k = B F;  cov' = F_k cov F_k^T
 * (tune/utils.py:441-471 + simulation_utils.py:25-48 in one pass; F_k never reaches HBM unless F_out != NULL). */
int nm_bind_frame(int32_t k, const int32_t* rowptr, const int32_t* col, const float* val,
                  const float* p_cur, const float* p_prev, const float* k_prev, const float* F,
                  const float* cov6, float* means3D, float* cov6_out, float* F_out, void* stream);

/* ------------------------------------------------------------------ rasterizer (diff_gaussian_rasterization) */

/* GaussianRasterizationSettings as filled by modules/d3gs/gaussian_renderer/__init__.py:103-116.
 * tile_y0/tile_y1: half-open range of 16-pixel tile rows this call renders (0,0 = whole image);
 * used to shard one view across GPUs. */
typedef struct nm_raster_cfg {
  int32_t image_height;
  int32_t image_width;
  float tanfovx;
  float tanfovy;
  float bg[3];
  float scale_modifier;
  float viewmatrix[16];
  float projmatrix[16];
  int32_t sh_degree;
  float campos[3];
  int32_t prefiltered;
  int32_t debug;
  int32_t tile_y0;
  int32_t tile_y1;
  int32_t split_items;   /* capacity, in (tile, list segment) work items, of the split compositing's records inside the
                          * state buffer (256 x 16 B kept for the backward pass + 256 x 36 B of forward scratch per item);
                          * 0 = 8192.  A view that wants more composites its remaining tiles whole: slower, same result;
                          * nm_raster_forward_ex reports what the view asked for */
} nm_raster_cfg;

/* One caller-allocated state buffer per rendered view replaces the geomBuffer / binningBuffer / imgBuffer tensors of the
 * reference extension (diff_gaussian_rasterization rasterize_points.cu, called from gaussian_renderer/__init__.py:103-119);
 * it is what the backward pass needs and nothing else.  cap_pairs = capacity, in (Gaussian, 64x64-pixel bin) pairs, of the
 * depth-sorted bin lists inside it (a Gaussian of the usual size touches 1-4 bins; 8 * k is a generous first guess). */
size_t nm_raster_state_bytes(const nm_raster_cfg* cfg, int32_t k, int64_t cap_pairs);

/* GaussianRasterizer.forward: preprocess, binning into (bin, depth slab) cells, per-cell LDS depth sort, per-tile
 * streaming composite -> out_color (3,H,W) and radii (K).  shs (K,M,3) or colors_precomp (K,3): exactly one non-NULL.
 * cov3D (K,6) required.  Rows outside the cfg tile stripe are left untouched.  Entirely asynchronous on `stream` (the
 * reference extension synchronises once per view to size its sort buffers).
 * status_host: NULL, or PINNED host memory of two zero-initialised int64 that receive, in stream order, {number of
 * pairs binned, overflow flag}.  overflow != 0: cap_pairs was too small, the image is incomplete - re-run with a state
 * buffer of capacity >= the reported number of pairs. */
int nm_raster_forward(const nm_raster_cfg* cfg, int32_t k, int32_t m, const float* means3D,
                      const float* shs, const float* colors_precomp, const float* opacities,
                      const float* cov3D, int32_t* radii, void* state, size_t state_bytes, int64_t cap_pairs,
                      float* out_color, int64_t* status_host, void* stream);
/* The same with (a) the forward-only arrays in a buffer of their own and (b) a per-camera walk record.
 * (a) nm_raster_state_bytes_ex splits what nm_raster_state_bytes adds up: *state_bytes = what the backward pass reads again
 * (keep it until then), *scratch_bytes = what only the forward pass uses (pair log, cell counters, per-segment scratch: the
 * larger half) - free it, or hand it to the next render on the same stream, as soon as the call has been enqueued.
 * scratch == NULL: one-buffer layout as in nm_raster_forward (state_bytes >= the sum).  nm_raster_count_pairs needs that
 * layout.
 * (b) tile_walk: NULL, or device memory of one uint32 per 16x16 tile of the image (ceil(W/16) * ceil(H/16), row-major),
 * zeroed by the caller when the camera is created and then handed to every render with that camera (the reference keeps
 * no state between two calls of the rasterizer, gaussian_renderer/__init__.py:103-119; this is an addition underneath
 * it).  The forward pass leaves in it how far along its depth-sorted list each tile had to walk, and plans the NEXT render
 * with the same camera from it: tiles with a long walk are cut into segments that are composited in parallel (forward and
 * reverse sweep), however many busy tiles the view has.  A stale or wrong record costs time, never accuracy: image,
 * termination rule and gradients are those of nm_raster_forward.
 * status_host: NULL or pinned memory of THREE zero-initialised int64: {pairs binned, overflow flag, work items the split
 * compositing asked for (compare with cfg.split_items)}. */
int nm_raster_state_bytes_ex(const nm_raster_cfg* cfg, int32_t k, int64_t cap_pairs, size_t* state_bytes,
                             size_t* scratch_bytes);
int nm_raster_forward_ex(const nm_raster_cfg* cfg, int32_t k, int32_t m, const float* means3D,
                         const float* shs, const float* colors_precomp, const float* opacities,
                         const float* cov3D, int32_t* radii, void* state, size_t state_bytes, void* scratch,
                         size_t scratch_bytes, int64_t cap_pairs, float* out_color, int64_t* status_host,
                         uint32_t* tile_walk, void* stream);
/* Tuning of the hinted plan (process-wide).  forward_split_length: tiles whose planned walk is longer than this many list
 * entries are composited in parallel segments in the forward pass as well; shorter ones are walked front to back (leaving
 * checkpoints) and only their reverse sweep runs in segments.  min_segment: shortest segment (rounded up to a multiple of
 * 16).  Defaults 0 (every planned tile: measured best for forward + backward together) and 256. */
int nm_raster_set_hinted(int32_t forward_split_length, int32_t min_segment);
/* Reverse compositing with two pixels per lane (process-wide; read by the following nm_raster_backward calls): pays when
 * several views' reverse sweeps share the chip, costs latency for a view that has it to itself.  Default 0.  Same gradients.
 * (Underneath the reference's stateless rasterizer interface, like the two knobs around it: no counterpart there.) */
int nm_raster_set_reverse_px2(int32_t on);
/* Tuning of the split compositing (process-wide; read by the following nm_raster_forward calls).  A view with fewer than
 * `busy_tiles` non-empty tiles leaves most of the chip idle; its tiles whose depth-sorted list is longer than a segment
 * (>= `min_segment` entries, ~4096 segments per view at most) are walked segment by segment on separate workgroups:
 * always in the reverse sweep (from checkpoints the forward pass leaves in front of every segment), and in the forward
 * pass for the tiles that still have a barely covered pixel after their first segment, provided the view's candidate
 * lists hold no more than `forward_budget` entries together (every segment of such a tile is composited, also those
 * behind the point where its pixels stop).  Same image, same termination rule (forward.cu: stop when T would fall below
 * 1e-4), same gradients.  Defaults 512 (two tiles per CU) / 512 / 2^21; busy_tiles = 0 switches the splitting off,
 * forward_budget = 0 keeps the forward walk sequential.  min_segment is rounded up to a multiple of 16. */
int nm_raster_set_split(int32_t busy_tiles, int32_t min_segment, int64_t forward_budget);
/* Exact number of (Gaussian, 16x16 tile) pairs of the view held in `state` - the `num_rendered` the reference extension
 * returns.  Statistics (byte accounting); synchronises `stream`. */
int nm_raster_count_pairs(const nm_raster_cfg* cfg, int32_t k, void* state, int64_t cap_pairs,
                          int64_t* pairs_out, void* stream);
/* GaussianRasterizer.backward.  dL_dcolor (3,H,W) in; outputs (any may be NULL except dL_dmeans3D):
 * dL_dmeans3D (K,3), dL_dmeans2D (K,3; screen-space mean gradient as the reference returns it),
 * dL_dcov3D (K,6), dL_dopacity (K,1), dL_dshs (K,M,3) or dL_dcolors (K,3).
 * state / cap_pairs: as passed to nm_raster_forward.  workspace: device scratch of nm_raster_bwd_workspace(k) bytes. */
size_t nm_raster_bwd_workspace(int32_t k);
int nm_raster_backward(const nm_raster_cfg* cfg, int32_t k, int32_t m, const float* means3D,
                       const float* shs, const float* colors_precomp, const float* opacities,
                       const float* cov3D, const void* state, int64_t cap_pairs, const float* dL_dcolor,
                       float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dcov3D, float* dL_dopacity,
                       float* dL_dshs, float* dL_dcolors, void* workspace, size_t workspace_bytes,
                       void* stream);

/* Fused pixel loss on the rendered image (modules/d3gs/utils/loss_utils.py:17-24):
 * kind 0 = l1 (mean |a-b|), 1 = l2 (mean (a-b)^2); *loss_out (device float) += weight * loss;
 * dL_dimg (3,H,W) = weight * dloss/dimg.  Rows outside [row0,row1) contribute nothing (sharded render). */
int nm_pixel_loss(int32_t kind, float weight, int32_t h, int32_t w, int32_t row0, int32_t row1,
                  const float* img, const float* gt, float* loss_out, float* dL_dimg, void* stream);

/* ------------------------------------------------------------------ Gaussian registration (experiments/regist.py) */

/* Register.forward (modules/tune/regist/register.py) + the covariance build (general_utils.py:93-139) for K Gaussians,
 * one pass.  params (DEVICE, 20 floats): R[9] (row-major), q_R[4] (wxyz), s, t[3], o[3]; xyz (K,3), log_scales (K,3),
 * rot (K,4) as loaded (normalised here, F.normalize).  Writes
 *   means3D = R (s (xyz - o)) + t,   log_scales' = log_scales + log s,
 *   rot'    = normalize(quaternion_multiply(normalize(rot), q_R))          (transform_utils.py:14-23, 218),
 *   cov6    = strip_symmetric(L L^T), L = build_rotation(rot') diag(scale_modifier exp(log_scales')).
 * out_log_scales / out_rot may be NULL. */
int nm_regist_apply(int32_t k, const float* xyz, const float* log_scales, const float* rot, const float* params,
                    float scale_modifier, float* means3D, float* cov6, float* out_log_scales, float* out_rot, void* stream);

/* Adjoint of nm_regist_apply, reduced over the K Gaussians: dL_dparams (DEVICE, 17 floats: dR[9], dq_R[4], ds, dt[3])
 * += sum_i of the per-Gaussian chain (R and q_R are independent inputs).  Two-stage, fixed-order reduction with fp64
 * partials: bitwise reproducible.  workspace: nm_regist_bwd_workspace(k) bytes of device scratch. */
size_t nm_regist_bwd_workspace(int32_t k);
int nm_regist_backward(int32_t k, const float* xyz, const float* log_scales, const float* rot, const float* params,
                       float scale_modifier, const float* dL_dmeans3D, const float* dL_dcov6, float* dL_dparams,
                       void* workspace, size_t workspace_bytes, void* stream);

/* The activations of a 3DGS parameter set (gaussian_model.py:26-41), one pass over K Gaussians: log_scales (K,3), rot (K,4)
 * raw (normalised here, 16-byte aligned), opacity_logit (K,1).
 *   cov6    = strip_symmetric(L L^T), L = build_rotation(normalize(rot)) diag(scale_modifier exp(log_scales))
 *   opacity = sigmoid(opacity_logit)
 * Either output may be NULL (its inputs may then be NULL too). */
int nm_gaussian_activate(int32_t k, const float* log_scales, const float* rot, const float* opacity_logit,
                         float scale_modifier, float* cov6, float* opacity, void* stream);
/* Its adjoint per Gaussian: dL_dlog_scales (K,3), dL_drot (K,4, through the normalisation) from dL_dcov6 (K,6), and
 * dL_dopacity_logit (K,1) from dL_dopacity (K,1).  Outputs are overwritten, not accumulated; any of them may be NULL. */
int nm_gaussian_activate_backward(int32_t k, const float* log_scales, const float* rot, const float* opacity_logit,
                                  float scale_modifier, const float* dL_dcov6, const float* dL_dopacity,
                                  float* dL_dlog_scales, float* dL_drot, float* dL_dopacity_logit, void* stream);

/* The raw 3DGS parameters of K deformed Gaussians (what a .ply of a rolled-out frame holds): log_scales (K,3) and rot (K,4) raw,
 * (r,x,y,z), 16-byte aligned, as nm_gaussian_activate reads them; F (K,3,3) row-major, or NULL for the identity (bitwise the
 * explicit identity).  log_scales_out (K,3) and rot_out (K,4, unit, r >= 0, 16-byte aligned) satisfy
 *   nm_gaussian_activate(log_scales_out, rot_out, scale_modifier = 1).cov6
 *     == strip_symmetric(F L L^T F^T), L = build_rotation(normalize(rot)) diag(scale_modifier exp(log_scales))
 * so the scale modifier is baked in.  Method: M = F L = U diag(s) V^T by the library's one-sided Jacobi SVD (U in SO(3) also for
 * det F < 0); the scales are |s_i|, the rotation is U (Shepperd's branch to the quaternion, normalised, sign fixed).  cov' is
 * never eigen-decomposed: that would square the condition number.
 * Every output is finite for every finite input whose product F L stays in the fp32 range.  A singular or zero F is legitimate:
 * each scale is clamped from below at max(1e-20 s_0, 1e-37) before the logarithm (s_0 the largest scale), i.e. at 1e-20 s_0, and
 * at 1e-37 where s_0 is zero or so small that 1e-20 s_0 lies below it.
 * The outputs may not overlap the inputs or each other: NM_ERR_INVALID.  No workspace. */
int nm_gaussian_deform(int32_t k, const float* log_scales, const float* rot, const float* F, float scale_modifier,
                       float* log_scales_out, float* rot_out, void* stream);

/* SH colour coefficients rotated with the Gaussians (transform_shs_by_rotmat, modules/d3gs/utils/transform_utils.py:41-104):
 * shs_out[g, :, ch] = diag(1, D_1, D_2, D_3)(R) shs_in[g, :, ch], D defined by sum_j c'_j Y_j(R d) = sum_j c_j Y_j(d) for
 * the rasterizer's basis Y, built from R as a polynomial (sh_rotation_matrices of render/transform_utils.py is the same
 * formula).  R: 9 DEVICE floats, row-major, as in `points @ R^T` (= params[0:9] of nm_regist_apply).  shs (k, n_coeff, 3):
 * n_coeff = 4 | 9 | 16 with has_dc = 1 (row 0, the DC term, is copied) or 3 | 8 | 15 with has_dc = 0 (a bare
 * _features_rest); any other count is NM_ERR_INVALID.  shs_out may alias shs_in. */
int nm_sh_rotate(int32_t k, int32_t n_coeff, int32_t has_dc, const float* R, const float* shs_in, float* shs_out, void* stream);

/* Adjoint of nm_sh_rotate: dL_dR (9 DEVICE floats) += sum over the Gaussians and channels, chained from the <= 83 entries of
 * dL/dD through the polynomial; dL_dshs_in (k, n_coeff, 3) = D^T dL_dshs_out (DC row copied), may be NULL, may alias
 * dL_dshs_out.  fp64 partials per workgroup, summed by one workgroup in a fixed order, no atomics: bitwise reproducible.
 * workspace: nm_sh_rotate_bwd_workspace(k) bytes of device scratch. */
size_t nm_sh_rotate_bwd_workspace(int32_t k);
int nm_sh_rotate_backward(int32_t k, int32_t n_coeff, int32_t has_dc, const float* R, const float* shs_in,
                          const float* dL_dshs_out, float* dL_dR, float* dL_dshs_in, void* workspace, size_t workspace_bytes,
                          void* stream);

/* SH colour coefficients rotated with each Gaussian's own deformation: as nm_sh_rotate (same basis, sample directions,
 * A_l^{-1}, n_coeff / has_dc rule), with one rotation per Gaussian, R_g = U V^T of the project's 3x3 SVD of F_g (nm_svd3_fwd's:
 * U, V in SO(3), the sign on sigma_2), the rotation part of the polar decomposition and a proper rotation also where
 * det F < 0.  F (k,3,3) row-major.  R_out: NULL, or (k,3,3), the rotation that was applied.  For a singular or zero F the
 * polar rotation is not defined: R_out is still what the SVD gives and every output is finite.  shs_out must not be shs_in
 * (NM_ERR_INVALID).  No reference counterpart: the reference hands the coefficients to the rasterizer unrotated. */
int nm_sh_rotate_polar(int32_t k, int32_t n_coeff, int32_t has_dc, const float* F, const float* shs_in, float* shs_out,
                       float* R_out, void* stream);

/* SSIM loss (modules/d3gs/utils/loss_utils.py:26-66, window 11, sigma 1.5, zero padding, size_average) of two (3,H,W) fp32
 * images: *loss_out (device float) += weight * (1 - ssim(img, gt)); dL_dimg (may be NULL) += weight * d(1 - ssim)/dimg.
 * Adds to both, so it composes with nm_pixel_loss called first.  The loss value is deterministic (fixed-order fp64
 * reduction).  workspace: nm_ssim_workspace(h, w) bytes of device scratch. */
size_t nm_ssim_workspace(int32_t h, int32_t w);
int nm_ssim_loss(float weight, int32_t h, int32_t w, const float* img, const float* gt, float* loss_out, float* dL_dimg,
                 void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ particle-state loss (neuma_amd/pretrain.py) */

/* Position + velocity loss of one frame against a recorded trajectory, fused with its gradient.  No reference counterpart
 * (the reference ships its base models, not their training).  x, v, x_gt, v_gt (n,3) fp32; mask NULL (all rows) or n bytes,
 * a row is kept where mask != 0; m = kept rows.  kind 0 = l1, 1 = l2:
 *   term_x = sum over kept rows and 3 components of |x - x_gt| (l1) or (x - x_gt)^2 (l2), divided by 3 m   (F.l1_loss /
 *   F.mse_loss over the kept rows), term_v likewise;  *loss_out (device float) += weight_x term_x + weight_v term_v;
 *   terms_out (NULL or 2 device floats) = {term_x, term_v}, unweighted, written;
 *   dL_dx = weight_x d(term_x)/dx, dL_dv = weight_v d(term_v)/dv: each NULL or (n,3), written (not added), 0 on rows the mask
 *   drops, and the l1 gradient is 0 where the difference is 0.
 * m == 0: the loss gains nothing, all gradients are 0.  v_gt == NULL: positions only, weight_v is ignored, v may be NULL and
 * dL_dv, if given, is written as zeros.  n == 0 is a no-op.  kind outside {0, 1}, a NULL x / x_gt / loss_out / workspace, v_gt
 * without v, or a workspace smaller than nm_state_loss_workspace(n) (device scratch, 8-byte aligned): NM_ERR_INVALID.
 * Differences and sums in fp64, per-workgroup partials summed by one workgroup in a fixed order, no float atomics: two calls
 * give identical bits, and so do 16-byte aligned operands (float4 path) and unaligned ones (scalar path). */
size_t nm_state_loss_workspace(int32_t n);
int nm_state_loss(int32_t n, int32_t kind, float weight_x, float weight_v, const float* x, const float* v, const float* x_gt,
                  const float* v_gt, const uint8_t* mask, float* loss_out, float* terms_out, float* dL_dx, float* dL_dv,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ Chamfer loss (neuma_amd/pretrain.py, loss: chamfer) */

/* Chamfer loss of the simulated particles x (n,3) against an unordered observation y (m,3), fp32 on the device, fused with its
 * gradient in x.  No reference counterpart.  mask NULL (all rows) or n bytes: a row with 0 takes no part, neither as a query nor
 * as a candidate; k = kept rows.  a(i) = the nearest y of kept row i, b(j) = the nearest kept x row of y_j, both by nm_chamfer's
 * rule (fp64 distances from the fp32 coordinates, lexicographic minimum of (distance^2, index)).
 *   term_xy = (1/k) sum over kept i of |x_i - y_a(i)|^2,  term_yx = (1/m) sum over j of |y_j - x_b(j)|^2  (both always computed);
 *   *loss_out (device float) += weight_xy term_xy + weight_yx term_yx: the fp64 value rounded once to fp32, then added;
 *   terms_out (NULL or 2 device floats) = {term_xy, term_yx}, unweighted, written;
 *   dL_dx (NULL or (n,3), written) = (2 weight_xy / k)(x_i - y_a(i)) + (2 weight_yx / m) sum over {j: b(j) = i} of (x_i - y_j),
 *   exactly 0 on dropped rows;  y gets no gradient;
 *   idx_xy (NULL or n, DEVICE int64) = a(i), -1 on dropped rows;  idx_yx (NULL or m, DEVICE int64) = b(j) in the ORIGINAL row
 *   numbering of x.
 * k == 0: the loss gains nothing, terms 0, gradient 0, both index arrays -1.  A NaN / Inf coordinate makes *loss_out NaN and the
 * affected gradient rows NaN; indices stay in range and the call completes.  n < 1, m < 1, a NULL x / y / loss_out / workspace
 * or a workspace smaller than nm_chamfer_loss_workspace(n, m) (device scratch, 16-byte aligned; 0 = invalid sizes):
 * NM_ERR_INVALID before any device work.
 * Differences and sums in fp64, one fp32 rounding per output; the sum over the observations that chose a row runs in an order
 * fixed by their indices (stable sort by b, then per-row sums: a thread for a short row, a wave for a long one); no float
 * atomics: two calls give identical bits, an unaligned view the bits of an aligned copy, and a masked call the bits of the call
 * on the compacted cloud.  With a mask, k is read back to the host: that call synchronises the stream once (and cannot be
 * captured into a graph); without a mask there is no synchronisation. */
size_t nm_chamfer_loss_workspace(int32_t n, int32_t m);
int nm_chamfer_loss(int32_t n, int32_t m, const float* x, const float* y, const uint8_t* mask, float weight_xy, float weight_yx,
                    float* loss_out, float* terms_out, float* dL_dx, int64_t* idx_xy, int64_t* idx_yx, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ image-quality metrics (experiments/evaluation.py) */

/* torchmetrics' PeakSignalNoiseRatio and structural_similarity_index_measure (gaussian window 11, sigma 1.5, k1 0.01, k2 0.03,
 * data_range = max(preds range, target range), variances clamped at 0) of B images of (C,H,W) fp32 each, preds and target
 * contiguous (B,C,H,W) on the device.  Writes sse_out[b] (DEVICE, fp64) = sum of (preds - target)^2 over image b and, unless
 * ssim_out is NULL, ssim_out[b] (DEVICE, fp64) = the mean SSIM over image b's C x (H-10) x (W-10) windows lying inside it (what
 * torchmetrics' reflect pad + crop leaves).  range_per_image != 0: c1, c2 from each image's own range (one call per frame, as
 * evaluation.py); 0: from the batch-wide range (torchmetrics on a batched call).  H, W >= 11.  Fixed-order fp64 reductions, no
 * atomics, no host synchronisation: two calls give identical bits.  workspace: nm_image_metrics_workspace(b, c, h, w) bytes of
 * device scratch. */
size_t nm_image_metrics_workspace(int32_t b, int32_t c, int32_t h, int32_t w);
int nm_image_metrics(int32_t b, int32_t c, int32_t h, int32_t w, const float* preds, const float* target,
                     int32_t range_per_image, double* sse_out, double* ssim_out, void* workspace, size_t workspace_bytes,
                     void* stream);

/* LPIPS, the third number of experiments/evaluation.py: LearnedPerceptualImagePatchSimilarity(net_type='vgg', normalize=True).
 * For a, b (B,3,H,W) in [0,1]: x = (2 x - 1 - shift) / scale per channel (shift -0.030, -0.088, -0.188; scale 0.458, 0.448,
 * 0.450); VGG-16's 13 convolutions (3x3, zero padding 1, bias, ReLU) with a 2x2 / stride 2 / floor max-pool after convolutions
 * 2, 4, 7 and 10; taps after the ReLU of convolutions 2, 4, 7, 10, 13; per tap and pixel t^ = t / sqrt(1e-8 + sum_c t^2) and
 * d = sum_c w_c (a^_c - b^_c)^2; the value of a pair is the sum over the five taps of the mean of d over the tap's pixels.
 * Activations are CHANNELS-LAST, (N,H,W,C) fp32 contiguous, 16-byte aligned, everywhere below.  No atomics, no host
 * synchronisation, nothing read back; two calls give identical bits, and an image's result does not depend on its batch slot.
 *
 * nm_conv3x3_relu  y (N,H,W,Cout) = relu(conv3x3(x (N,H,W,Cin)) + bias).  Cout % 64 == 0; Cin == 3 (plain VALU) or
 *                  Cin % 16 == 0 (implicit GEMM on v_mfma_f32_16x16x4_f32, exact fp32: one fmaf chain over k per output, whose
 *                  order depends on Cin alone).  weight, packed from torch's (Cout,Cin,3,3) w: Cin == 3: (Cout, 9, 3) =
 *                  w[o][c][ky][kx] at [o][3 ky + kx][c]; otherwise (Cin/16, Cout, 9, 16) = w[o][16 j + c][ky][kx] at
 *                  [j][o][3 ky + kx][c].  y may not alias x.
 * nm_maxpool2      y (N,H/2,W/2,C) = 2x2 max-pool, stride 2, an odd last row / column dropped.  C % 4 == 0.
 * nm_lpips_head    out_fp64[p] (DEVICE) = the pixel mean of d for pair p of tap_a, tap_b (n_pairs,H,W,C), C % 4 == 0, head_w C
 *                  floats.  Norms, quotients and sums in fp64, the pixel sum in the fixed order of csrc/nm_reduce.h.
 *                  ws: nm_lpips_head_workspace(n_pairs, h, w) bytes of device scratch.
 * nm_lpips         the whole chain for B pairs: out_fp64[B] (DEVICE).  a, b_img: (B,3,H,W) fp32 planar, as images come.
 *                  weights: HOST array of 26 DEVICE pointers, packed weight then bias of each convolution in order; heads:
 *                  HOST array of 5 DEVICE pointers (64, 128, 256, 512, 512 floats).  ws: nm_lpips_workspace(b, h, w) bytes of
 *                  device scratch, 256-byte aligned (two activation buffers of 2B x H x W x 64 floats and small change).
 * NM_ERR_INVALID with nm_last_error text before any device work: H or W < 16 (nm_lpips; the workspace size is then 0), sizes
 * out of range, channel counts the kernels do not take, null or misaligned pointers, a workspace that is too small. */
int nm_conv3x3_relu(int32_t n, int32_t cin, int32_t cout, int32_t h, int32_t w, const float* x, const float* weight,
                    const float* bias, float* y, void* stream);
int nm_maxpool2(int32_t n, int32_t c, int32_t h, int32_t w, const float* x, float* y, void* stream);
size_t nm_lpips_head_workspace(int32_t n_pairs, int32_t h, int32_t w);
int nm_lpips_head(int32_t n_pairs, int32_t c, int32_t h, int32_t w, const float* tap_a, const float* tap_b, const float* head_w,
                  double* out_fp64, void* ws, size_t ws_bytes, void* stream);
size_t nm_lpips_workspace(int32_t b, int32_t h, int32_t w);
int nm_lpips(int32_t b, int32_t h, int32_t w, const float* a, const float* b_img, const float* const* weights,
             const float* const* heads, double* out_fp64, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ particle metrics (modules/tune/metrics.py) */

/* Exact 1-nearest-neighbour search, batched over b pairs of clouds: query (b, n_query, 3) and target (b, n_target, 3) fp32,
 * contiguous, on the device.  For every query point: idx_out[b][i] (DEVICE, int64) = the index of its nearest target and,
 * unless d2_out is NULL, d2_out[b][i] (DEVICE, fp64) = that squared distance.  Distances are fp64 from the fp32 coordinates;
 * the winner is the lexicographic minimum of (distance^2, target index), i.e. scipy cKDTree's fp64 choice except on exact
 * ties.  A query with a NaN / Inf coordinate gets index 0 and distance NaN.  Both clouds are binned per item into a uniform
 * grid over their own bounding box (found on the device); no atomics on floating-point values, no host synchronisation: two
 * calls give identical bits.  workspace: nm_nn_workspace(b, n_query, n_target) bytes of device scratch (0 = invalid sizes).
 * b < 1, an empty cloud or a too small workspace -> -1 before any device work. */
size_t nm_nn_workspace(int32_t b, int32_t n_query, int32_t n_target);
int nm_nearest_neighbors(int32_t b, int32_t n_query, int32_t n_target, const float* query, const float* target,
                         int64_t* idx_out, double* d2_out, void* workspace, size_t workspace_bytes, void* stream);
/* Exact k-nearest-neighbour search, 1 <= k <= 16, with the clouds, the binning and the distance arithmetic of
 * nm_nearest_neighbors: for every query the k targets with the smallest (distance^2, target index) in lexicographic order,
 * ascending.  idx_out (b, n_query, k) (DEVICE, int64); d2_out (b, n_query, k) (DEVICE, fp64) or NULL.  With k = 1 the result
 * equals nm_nearest_neighbors bit for bit.  exclude_same_index != 0 (query and target are the same cloud): target i is no
 * neighbour of query i - dropped by index, not by distance, so a coincident duplicate stays a neighbour at distance 0.  A query
 * with a NaN / Inf coordinate gets indices 0 and distances NaN (as does a slot for which no finite target is left).  The k best
 * are held in registers per thread; the walk stops once the k-th best squared distance is at most the squared distance to the
 * slab beyond each face of the visited block of cells.  No atomics on floating-point values, no host synchronisation: two calls
 * give identical bits.  workspace: nm_knn_workspace(b, n_query, n_target, k) bytes (0 = invalid sizes).  k out of range, fewer
 * than k eligible targets (n_target, less one with exclude_same_index) or a too small workspace -> -1 before any device work. */
size_t nm_knn_workspace(int32_t b, int32_t n_query, int32_t n_target, int32_t k);
int nm_knn(int32_t b, int32_t n_query, int32_t n_target, int32_t k, int32_t exclude_same_index, const float* query,
           const float* target, int64_t* idx_out, double* d2_out, void* workspace, size_t workspace_bytes, void* stream);
/* out[i] (DEVICE, fp32) = the mean of the k smallest squared distances from points[i] to the OTHER points of the cloud
 * (n, 3), excluded by index; the k fp64 distances are summed ascending in fp64 and the mean is rounded once.  k = 3 is the
 * documented behaviour of simple_knn's distCUDA2 (3DGS scale initialisation).  n - 1 < k -> -1.  workspace:
 * nm_knn_mean_dist2_workspace(n) bytes. */
size_t nm_knn_mean_dist2_workspace(int32_t n);
int nm_knn_mean_dist2(int32_t n, const float* points, int32_t k, float* out, void* workspace, size_t workspace_bytes,
                      void* stream);
/* Both directions of a Chamfer distance (metrics.py chamfer_distance_kdtree) in one call: p1 (b, n1, 3), p2 (b, n2, 3).
 * cd12_out[b] / cd21_out[b] (DEVICE, fp64) = the mean over p1 (p2) of the squared distance to its nearest point of p2 (p1),
 * fixed-order sums; NaN for an item where either cloud holds a NaN / Inf coordinate (other items are unaffected).
 * idx12 (b, n1) / idx21 (b, n2) (DEVICE, int64): the nearest-neighbour indices, or NULL.  workspace:
 * nm_chamfer_workspace(b, n1, n2) bytes. */
size_t nm_chamfer_workspace(int32_t b, int32_t n1, int32_t n2);
int nm_chamfer(int32_t b, int32_t n1, int32_t n2, const float* p1, const float* p2, double* cd12_out, double* cd21_out,
               int64_t* idx12, int64_t* idx21, void* workspace, size_t workspace_bytes, void* stream);

/* Earth mover's distance: an exact, bitwise repeatable linear assignment between clouds a (b, n, 3) and bb (b, n, 3) of n points
 * each (fp32, DEVICE), 1 <= n <= 8192, power 1 or 2.  No reference counterpart; neuma_amd/extras/emd.py is the numpy twin that
 * reproduces assignment, prices and round count bit for bit.  Per item:
 *   cost    c(i,j) = (dx*dx + dy*dy) + dz*dz in fp64 from the fp32 coordinates, in that order, no fma; power 1: its fp64 sqrt.
 *   scale   Cmax = the same expression on the extent of the joint bounding box; frexp(Cmax) = (m, ex), k = 24 - ex,
 *           C(i,j) = llrint(ldexp(c(i,j), k)) <= 2^24.  Cmax == 0 (all points identical): identity, emd 0, rounds 0, prices 0.
 *   solver  forward auction in Jacobi form with eps-scaling on Cs = C (n + 1), int64: prices start at 0, eps0 = max(1, max(Cs) / 2),
 *           eps <- max(1, eps / 4) per phase down to 1; a phase starts with nobody assigned and keeps the prices.  In a round every
 *           unassigned person i bids from one price snapshot: v_j = -Cs(i,j) - price_j, j* the lowest j of maximal v, w1 = v_j*,
 *           w2 = max over j != j* (w1 for n = 1), bid = price_j* + (w1 - w2) + eps; per object the highest bid wins, the lowest
 *           person among equal bids; the previous owner becomes unassigned and the price becomes the bid.
 *   value   emd_out[item] = mean_i c(i, idx(i)) from the unquantised fp64 costs (compensated sum, fixed order).
 * At eps = 1 the result satisfies 1-complementary slackness on Cs, so sum C(i,idx(i)) <= opt(C) + n / (n + 1): an exact optimum
 * of the quantised problem.  Therefore the reported value exceeds the true fp64 optimum by at most 2^-k <= Cmax * 2^-23.
 * idx_out (b, n) int64: person -> object.  price_out (b, n) int64 or NULL: the final prices on Cs.  rounds_out (b) int64: bidding
 * rounds.  One workgroup per item, the whole auction in one launch, every loop bounded by n or max_rounds; no n x n matrix.
 * An item with a NaN / Inf coordinate gets emd NaN, idx -1, rounds 0 (other items are unaffected; not an error).  An item that
 * is not finished after max_rounds rounds, or whose bid would reach 2^50 ("price overflow"), gets emd NaN, idx -1, rounds -1; the
 * kernel finishes normally and the call returns NM_ERR_LIMIT with a message naming the first such item.  The per-item status
 * words are read back: the call synchronises the stream once.  n outside 1..8192, power outside {1, 2}, max_rounds < 1, null
 * pointers or a workspace smaller than nm_emd_workspace(b, n) (0 = invalid sizes): NM_ERR_INVALID before any device work. */
size_t nm_emd_workspace(int32_t b, int32_t n);
int nm_emd(int32_t b, int32_t n, int32_t power, int64_t max_rounds, const float* a, const float* bb, double* emd_out,
           int64_t* idx_out, int64_t* price_out, int64_t* rounds_out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ mesh sampling (particles inside a triangle mesh) */

/* Ray-parity inside test of a triangle mesh, bit for bit the fp64 formula of extras/mesh_sampling.py points_in_mesh applied to
 * points that ALREADY carry its ray offset: verts (n_verts, 3) fp64, tris (n_tris, 3) int32, points (n_points, 3) fp64, all
 * contiguous on the device.  Triangles with |d| <= 1e-300 (d = twice the signed xy area) or a vertex index outside
 * [0, n_verts) are dropped (an out-of-range vertex is never read).  inside_out[i] (DEVICE, uint8) = 1 when the number of
 * triangles with barycentrics l0, l1, l2 >= 0 at the point's xy and interpolated z > the point's z is odd.  No float atomics,
 * no host synchronisation: two calls give identical bytes.  workspace: nm_mesh_inside_workspace(n_tris, n_points) bytes of
 * device scratch (0 = invalid sizes).  Negative sizes, n_tris > 2^27 or a too small workspace -> -1 before any device work. */
size_t nm_mesh_inside_workspace(int32_t n_tris, int32_t n_points);
int nm_points_in_mesh(int32_t n_verts, int32_t n_tris, int32_t n_points, const double* verts, const int32_t* tris,
                      const double* points, uint8_t* inside_out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ mesh distance field (no reference counterpart) */

/* Unsigned distance of the nodes of a regular lattice to a triangle mesh (kernels: csrc/nm_sdf.hip; the same definition in
 * numpy, fp64 and fp32: neuma_amd/extras/mesh_sdf.py, whose module docstring spells the per-triangle formula - closest point
 * by Voronoi region - operation by operation).  verts (n_verts, 3) fp32 and tris (n_tris, 3) int32 contiguous on the DEVICE;
 * origin (3 floats) and dims (3 ints) on the HOST.  dist_out[(ix ny + iy) nz + iz] (DEVICE, fp32) = the minimum over the kept
 * triangles of the distance from origin + (ix, iy, iz) spacing to the triangle, evaluated in fp32 without fma contraction and
 * with correctly rounded division and square root; +inf when no triangle is kept.  A triangle with a vertex index outside
 * [0, n_verts) is dropped and never read; a triangle whose squared area aa cc - bb^2 is not above 1e-6 aa cc (aa, bb, cc the
 * dot products of its two edges at the first vertex) counts as the union of its three edge segments, a zero-length segment
 * as a point.  Vertices are expected to be finite.  The minimum does not depend on the order of the triangles; no float
 * atomics, no host synchronisation: two calls give identical bytes.  workspace: nm_mesh_distance_workspace(n_tris, n_nodes)
 * bytes of device scratch (0 = invalid sizes).  -1 before any device work: negative sizes, n_tris > 2^24, a dim < 2, more
 * than 2^27 nodes, a spacing that is not positive and finite, a non-finite origin, a too small workspace. */
size_t nm_mesh_distance_workspace(int32_t n_tris, int64_t n_nodes);
int nm_mesh_distance(int32_t n_verts, int32_t n_tris, const float* verts, const int32_t* tris, const float* origin, float spacing,
                     const int32_t* dims, float* dist_out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ Gaussian fill (particles out of the density field) */

/* Particles from the opacity density of the Gaussians themselves (neuma_amd/gaussian_fill.py; extras/gaussian_fill.py states
 * the algorithm in numpy fp64 and computes the lattice for both).  Lattice: `origin` (3 HOST doubles, low corner of cell
 * (0,0,0)), cell edge h, `dims` (3 HOST ints, at most 2^27 cells); linear cell index (ix ny + iy) nz + iz.  The lattice is
 * cut into blocks of 4 x 4 x 4 cells, n_blocks = prod(ceil(dims / 4)).
 *   nm_fill_gaussians  per Gaussian, in fp64: inv(cov) by cofactors and the blocks under the box of its ellipsoid
 *                      m <= cutoff (half extent sqrt(cutoff cov_ii), clamped to the lattice).  g10 (K, 10) = mean, the six
 *                      unique entries of inv(cov) (xx xy xz yy yz zz), opacity; boxes (K, 6) int32 = low and high block per
 *                      axis; counts (K) int32 = blocks under the box.  A Gaussian whose determinant is not a positive
 *                      finite number (or whose inverse does not fit fp32) gets count 0 and opacity 0: it contributes
 *                      nothing.  totals (2 DEVICE int64) = {sum of counts, Gaussians skipped}: the caller reads them back.
 *   nm_fill_density    field (ncells, fp32): d(c) = sum over k with m_k <= cutoff of o_k exp(-m_k / 2) at every cell centre
 *                      c = origin + (i + 1/2) h (fp64, rounded to fp32 once), m_k = (c - mu_k)^T inv(cov_k) (c - mu_k) in
 *                      fp32.  The (block, Gaussian) pairs are sorted (rocPRIM) and one wave per block sums its list in
 *                      ascending Gaussian index: no float atomics, two calls give identical bytes; every cell is written.
 *                      n_pairs = totals[0], below 2^31.  workspace: nm_fill_density_workspace(K, n_pairs, n_blocks) bytes
 *                      (0 = invalid sizes).
 *   nm_fill_classify   on ANY field: kind_cell (ncells, uint8) = 1 where field > density_thres (shell), 2 where not, and on
 *                      each of the three axis lines through the cell there is a shell cell at a strictly lower and one at
 *                      a strictly higher index (enclosed), else 0.  Kept = enclosed, plus shell when include_shell.
 *                      offsets (ncells, int32) = number of kept cells before each cell; counts (3 DEVICE int32) = {kept,
 *                      shell, enclosed}: the caller reads them back to size the output.  workspace:
 *                      nm_fill_classify_workspace(dims) bytes.
 *   nm_fill_emit       per kept cell, in ascending linear index, per_cell^3 points origin_a + (i_a + (s_a + 1/2) / per_cell) h,
 *                      s nested x, y, z, each evaluated in fp64 by that expression and rounded to fp32 once:
 *                      points (n_kept per_cell^3, 3) fp32, kind_out (n_kept per_cell^3) uint8 (1 shell, 2 enclosed).
 * Invalid sizes or a too small workspace fail before any device work; no entry synchronises with the host. */
int nm_fill_gaussians(int32_t K, const float* means, const float* cov6, const float* opacity, const double* origin, double h,
                      const int32_t* dims, float cutoff, float* g10, int32_t* boxes, int32_t* counts, int64_t* totals,
                      void* stream);
size_t nm_fill_density_workspace(int32_t K, int64_t n_pairs, int32_t n_blocks);
int nm_fill_density(int32_t K, int64_t n_pairs, const float* g10, const int32_t* boxes, const int32_t* counts,
                    const double* origin, double h, const int32_t* dims, float cutoff, float* field, void* workspace,
                    size_t workspace_bytes, void* stream);
size_t nm_fill_classify_workspace(const int32_t* dims);
int nm_fill_classify(const int32_t* dims, const float* field, float density_thres, int32_t include_shell, uint8_t* kind_cell,
                     int32_t* offsets, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int nm_fill_emit(const int32_t* dims, const double* origin, double h, int32_t per_cell, int32_t include_shell,
                 const uint8_t* kind_cell, const int32_t* offsets, int64_t n_kept, float* points, uint8_t* kind_out,
                 void* stream);

/* ------------------------------------------------------------------ surface meshes (no reference counterpart) */

/* A closed, consistently oriented, indexed triangle mesh of the level set {f = iso} of a lattice field (neuma_amd/surface_mesh.py;
 * extras/surface_mesh.py states the algorithm - marching tetrahedra on the Kuhn subdivision - in numpy fp64 and is the CPU path).
 * `field` (ncells, fp32, DEVICE) in the layout of nm_fill_density: linear index (ix ny + iy) nz + iz, sample i at
 * origin + (i + 1/2) h; `dims` 3 HOST ints, at most 2^27 cells; iso finite and > 0; a sample is inside iff f >= iso.  The
 * lattice is extended by one ring of samples of value 0 on every side: extended dims E = dims + 2, extended sample e = i + 1,
 * NE = E0 E1 E2, linear index (ex E1 + ey) E2 + ez.  Every extended sample owns the 7 edges to its neighbours +x, +y, +z, +x+y,
 * +y+z, +x+z, +x+y+z (slots 0 .. 6) and the cube between itself and e + (1,1,1), cut into the six tetrahedra
 * 000 -> e_p0 -> e_p0 + e_p1 -> 111 of the axis permutations p in lexicographic order.
 *   nm_surface_count  mask (NE, uint8): bit s set where the ends of slot s differ in the inside test; tri_count (NE, uint8):
 *                     triangles of the sample's cube (0 .. 12); vert_offset / tri_offset (NE, int32): exclusive prefix sums of
 *                     popcount(mask) and tri_count in ascending extended index; info (3 DEVICE int64) = {V, T, non-finite flag}:
 *                     the caller reads them back, refuses a non-zero flag and totals beyond int32 (the 32-bit offsets are then
 *                     meaningless), and sizes the outputs.  One pass over the field: a workgroup stages a brick of samples with
 *                     its +1 halo in LDS.  workspace: nm_surface_workspace(dims) bytes of device scratch (0 = invalid dims).
 *   nm_surface_emit   the vertex of (sample, slot) lands at vert_offset[sample] + popcount(mask below slot):
 *                     vertices (V, 3) fp32 = p_a + t (p_b - p_a), t = (iso - f_a) / (f_b - f_a) in fp32 with a the owning
 *                     sample, the end points and the product in fp64 from `origin` (3 HOST doubles) and h, rounded to fp32
 *                     once; normals (V, 3) = the normalised negative gradient, central differences at the two ends (0 outside
 *                     the real lattice) interpolated with t, (0, 0, 0) for a zero gradient; vertex_attrs (V, n_attrs) from
 *                     attrs (n_attrs <= 4, ncells; may be NULL with n_attrs = 0), a ring sample carrying the nearest real
 *                     sample's value.  triangles (T, 3) int32 at tri_offset[cube], by tetrahedron, wound so that the normal
 *                     points from inside to outside; zero-area triangles (a sample equal to iso) are kept, so the surface is
 *                     closed on any finite field.  An offset outside [0, V) / [0, T) is never written through.
 * Integer sums only: two calls give identical bytes.  Invalid dims, iso, h, origin, counts, a null pointer or a too small
 * workspace fail before any device work; no entry synchronises with the host. */
size_t nm_surface_workspace(const int32_t* dims);
int nm_surface_count(const int32_t* dims, const float* field, float iso, uint8_t* mask, uint8_t* tri_count, int32_t* vert_offset,
                     int32_t* tri_offset, int64_t* info, void* workspace, size_t workspace_bytes, void* stream);
int nm_surface_emit(const int32_t* dims, const double* origin, double h, const float* field, float iso, int32_t n_attrs,
                    const float* attrs, const uint8_t* mask, const uint8_t* tri_count, const int32_t* vert_offset,
                    const int32_t* tri_offset, int64_t n_verts, int64_t n_tris, float* vertices, float* normals,
                    float* vertex_attrs, int32_t* triangles, void* stream);

/* ------------------------------------------------------------------ classical constitutive laws (material/classical.py) */

/* The closed-form laws of the reference's nclaw/material/preset.py:30-282, one thread per particle.  `law`: */
#define NM_LAW_COROTATED 0      /* stress  2 mu (F - U Vh) F^T + la J (J - 1) I,  J = prod(sigma) */
#define NM_LAW_STVK 1           /* stress  mu F (F^T F - I) + la J (J - 1) I,     J = prod(sigma) */
#define NM_LAW_VOLUME 2         /* stress  mode 0 (ziran): kappa (J - 1 / J) I;  mode 1 (taichi): la J (J - 1) I;  J = det F */
#define NM_LAW_SIGMA 3          /* stress  U diag(2 mu log sigma + la tr log sigma) U^T (NaN where a sigma is negative) */
#define NM_LAW_IDENTITY 4       /* F       a device-to-device copy, no kernel */
#define NM_LAW_SIGMA_PLASTIC 5  /* F       diag(det(F)^(1/3)) (NaN where det F < 0) */
#define NM_LAW_VON_MISES 6      /* F       sigma clamped at 0.05, return map where |dev log sigma| > sigma_y / (2 mu), else F */
#define NM_LAW_DRUCKER_PRAGER 7 /* F       sigma clamped at 0.05; cone projection where tr log sigma < 3 cohesion, else exp(cohesion) U Vh */
#define NM_VOLUME_ZIRAN 0
#define NM_VOLUME_TAICHI 1
/* scalars (DEVICE, 4 floats, read by the kernel - no host copy): {log_E, nu, p2, p3} with p2 = sigma_y (law 6) or the friction
 * angle in degrees (law 7) and p3 = cohesion (law 7); unused entries are ignored (laws 4, 5 accept NULL).  F, out: (n, 3, 3)
 * fp32 row-major.  The SVD is nm_svd3_fwd's.  Both branches of a switch are evaluated and selected, so a row with
 * |dev log sigma| = 0 gives what the reference gives (NaN on the yielding side of law 7). */
int nm_classical_fwd(int32_t n, int32_t law, int32_t mode, const float* scalars, const float* F, float* out, void* stream);
/* Adjoint: grad_F (n, 3, 3), and grad_scalars (DEVICE, 2 floats, OVERWRITTEN: {d/d log_E, d/d p2}; may be NULL for laws 4, 5)
 * summed over the particles as fp64 per-block partials and one fixed-order block (no float atomics: two calls give the same
 * bits).  The SVD is recomputed; its adjoint is nm_svd3_bwd's clamped form.  Where a switch picks the other branch that
 * branch's gradient is dropped by a select, not multiplied by zero: a non-yielding von Mises row with |dev log sigma| = 0
 * returns grad_out (the reference returns NaN there).  Non-finite values are passed on unchanged.
 * workspace: nm_classical_bwd_workspace(n) bytes of device scratch (0 for n <= 0). */
size_t nm_classical_bwd_workspace(int32_t n);
int nm_classical_bwd(int32_t n, int32_t law, int32_t mode, const float* scalars, const float* F, const float* grad_out,
                     float* grad_F, float* grad_scalars, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ field paint (no reference counterpart) */

/* Colouring a roll-out by a per-particle quantity (kernels: csrc/nm_paint.hip, per-particle body: csrc/nm_particle_field.h; the
 * same definitions in torch fp64: neuma_amd/extras/field_paint.py, which is also the CPU path).  Four steps:
 *
 * 1. Per-particle quantity q from x, v (n, 3), F, the Kirchhoff stress tau = elasticity(F) (n, 3, 3 row-major) and the initial
 *    position x0 (n, 3); J = det F: */
#define NM_FIELD_SPEED 0        /* |v| */
#define NM_FIELD_DISPLACEMENT 1 /* |x - x0| */
#define NM_FIELD_VOLUME 2       /* J */
#define NM_FIELD_STRAIN 3       /* Hencky equivalent strain: e_i = log(max(|s_i|, 1e-20)), s = nm_svd3(F), m = mean(e),
                                   q = sqrt(2/3 sum_i (e_i - m)^2) */
#define NM_FIELD_PRESSURE 4     /* -tr(tau) / (3 J); NaN where J <= 0 */
#define NM_FIELD_VON_MISES 5    /* sigma = (tau + tau^T) / (2 J), d = sigma - tr(sigma) / 3 I, q = sqrt(3/2 sum_ab d_ab^2);
                                   NaN where J <= 0 */
#define NM_FIELD_COUNT 6
/*    A NaN or Inf in an array the quantity reads gives a non-finite q.  Non-finite means "no data" in every later step.
 *
 * 2. Per-Gaussian value over the binding CSR (rowptr (K + 1), col, val: tune.Bindings):
 *      g_k = (sum_j val_kj q[col_kj]) / (sum_j val_kj), over the row in CSR order, both sums in fp32;
 *    NaN for an empty row, a weight sum of 0, a bound q that is non-finite, and a column index outside [0, n) (never read).
 *
 * 3. Range [lo, hi], hi > lo: the caller's, or the minimum and maximum over the finite g_k.  When that gives hi <= lo the range
 *    is [lo, lo + 1], and [0, 1] when there is no finite value.
 *
 * 4. Colour: t = clamp((g - lo) / (hi - lo), 0, 1); a colour map is n_knots rgb knots c_0 .. c_{n-1} at equal spacing,
 *    2 <= n_knots <= NM_PAINT_MAX_KNOTS:  i = min(floor(t (n - 1)), n - 2),  u = t (n - 1) - i,  rgb = c_i + u (c_{i+1} - c_i).
 *    A non-finite g takes the no-data colour.  The output is the SH DC coefficient (rgb - 1/2) / C0, C0 = 0.28209479177387814
 *    (the rasterizer's), so a Gaussian rendered at sh_degree 0 shows exactly rgb. */
#define NM_PAINT_MAX_KNOTS 8

/* Step 1, one particle per lane; q_out (n) fp32 on the DEVICE.  Arrays the quantity does not read may be NULL (speed: v;
 * displacement: x, x0; volume, strain: F; pressure, von_mises: F, stress); one it reads may not (-1, the message names it), nor
 * may q_out.  n == 0 is a no-op; n < 0 or an unknown quantity -> -1 before any device work. */
int nm_particle_field(int32_t n, int32_t quantity, const float* x, const float* v, const float* F, const float* stress,
                      const float* x0, float* q_out, void* stream);
/* Step 3 on the device: the minimum and maximum of the finite values of g (k, fp32) by one fixed-order reduction (no float
 * atomics, no host read-back; both are exact, so two calls give identical bits).  range_inout: 2 DEVICE floats {lo, hi}.
 * mode 0 writes the frame's range with the widening rule of step 3.  mode 1 folds the frame's finite minimum / maximum into the
 * pair already there (start it at {+inf, -inf}; nothing is widened): the overall range of a sequence.  k == 0 counts as "no
 * finite value".  workspace: nm_field_range_workspace(k) bytes of device scratch (0 for k < 0). */
size_t nm_field_range_workspace(int32_t k);
int nm_field_range(int32_t k, const float* g, float* range_inout, int32_t mode, void* workspace, size_t workspace_bytes,
                   void* stream);
/* Steps 2 and 4, one Gaussian per lane: q (n) and range_dev (2 floats {lo, hi}) on the DEVICE - a range found by nm_field_range
 * costs no synchronisation; knots (3 n_knots floats) and nodata_rgb (3 floats) on the HOST.  g_out (k) and dc_out (k, 3) fp32
 * on the DEVICE; either may be NULL (not written; range_dev and the map are then not needed for a call without dc_out), not
 * both.  rowptr == NULL paints q itself: g = q, which needs k == n (the particle-colour export).  A range with hi <= lo or a
 * non-finite bound paints everything in the no-data colour. */
int nm_field_paint(int32_t k, int32_t n, const int32_t* rowptr, const int32_t* col, const float* val, const float* q,
                   const float* range_dev, int32_t n_knots, const float* knots, const float* nodata_rgb, float* g_out,
                   float* dc_out, void* stream);

/* ------------------------------------------------------------------ driven meshes (no reference counterpart) */

/* A user's triangle mesh carried along by the particles (neuma_amd/mesh_drive.py; extras/mesh_drive.py states the definition in
 * numpy fp64 and is the CPU path).  A vertex follows its k nearest rest particles (1 <= k <= 16) by an affine moving-least-squares
 * fit written as fixed coefficients, so a frame is one sparse product.
 *   nm_mesh_bind     idx (n_verts, k) int64 / d2 (n_verts, k) fp64 (DEVICE): the lists of nm_knn (query = verts, target = particles),
 *                    ascending.  Per vertex, in fp64, every sum over j = 0 .. k-1 in that order:
 *                      R2 = 1.21 d2_{k-1};  w_j = (1 - d2_j / R2)^2 (1 when R2 == 0);  w^_j = w_j / sum w_j
 *                      Xbar = sum w^_j X_j (summed as X_0 + sum w^_j (X_j - X_0));  y_j = X_j - Xbar;  M = sum w^_j y_j y_j^T;  tau = tr M;  r = V0_v - Xbar
 *                      g = (M M + (damping tau)^2 I)^-1 M r  (0 when tau == 0; L D L^T on M / tau)
 *                      c_j = w^_j (1 + y_j . g)
 *                    col (n_verts, k) int32 = idx, coeff = c, weight = w^ (n_verts, k) fp32, each rounded once.  The rows are a
 *                    CSR with rowptr = k arange(n_verts + 1): position = V0 + coeff (x - X) through nm_spmm_csr or nm_bind_frame,
 *                    vertex values through nm_field_paint over `weight`.  An index outside [0, n_particles) is never read through.
 *                    damping finite and > 0, n_particles >= k, n_verts k < 2^31.
 *   nm_mesh_normals  area-weighted vertex normals, fp32, no atomics, one pass.  vptr (n_verts + 1) / vcorner (3 n_tris) int32: the
 *                    corner ids 3 t + c sorted by (vertex, corner id).  Vertex v sums, over vcorner[vptr[v] .. vptr[v + 1]) in that
 *                    order, (p_next - p_v) x (p_prev - p_v) of the corner's triangle; a triangle with a repeated index or an index
 *                    outside [0, n_verts) adds zero and no position is read through it; the sum is scaled by its largest
 *                    |component| and normalised, (0, 0, 0) when it is zero or not finite.  3 n_tris < 2^31.
 * Both: null pointers and sizes out of range fail with NM_ERR_INVALID before any device work; n_verts == 0 is a no-op; no
 * synchronisation with the host; two calls give identical bits. */
int nm_mesh_bind(int32_t n_verts, int32_t n_particles, int32_t k, double damping, const float* verts, const float* particles,
                 const int64_t* idx, const double* d2, int32_t* col, float* coeff, float* weight, void* stream);
int nm_mesh_normals(int32_t n_verts, int32_t n_tris, const float* positions, const int32_t* triangles, const int32_t* vptr,
                    const int32_t* vcorner, float* normals_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NEUMA_HIP_H */
