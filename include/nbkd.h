/*
 * nbkd.h — C ABI of the MI355X-native kd-tree (libnbkd.so).
 *
 * Drop-in boundary for the reference's kd-tree hot path (wendazhou/nbodyhpc,
 * kdtree/ subsystem).  Plain pointers and sizes; no exceptions and no C++ or
 * torch types cross this boundary.  The pybind11 module nbodyhpc_amd.kdtree._impl
 * (mirror of kdtree/src/cpp/pybind.cpp) is one caller; a ctypes / cffi / JNI /
 * cgo stub is another.
 *
 * Ownership: the caller owns every input and output buffer; the library owns
 * the tree handle and everything on the device behind it.  Buffers are host
 * memory unless the matching NBKD_*_DEVICE flag is set, in which case they are
 * device pointers on the tree's device.  `stream` is a hipStream_t (NULL = the
 * null stream).  With host outputs a call returns after the results are
 * copied back.  With device outputs nbkd_query_knn / nbkd_query_kth return once
 * the work is enqueued (the re-walk of the queries whose seed ball held fewer
 * than k points runs on grids that read the failure count on the device), and
 * so does nbkd_query_ball_count.  nbkd_query_ball_csr waits (its offsets are
 * host memory), and the first call of a tree, or one needing more scratch than
 * any before it, may also wait while the scratch grows.  Calls on one tree
 * from several host threads run concurrently (the reference's query is const,
 * kdtree/src/cpp/pybind.cpp:90): a tree keeps up to 4 scratch workspaces and
 * each call holds one; a call reusing a workspace from another stream first
 * waits for that workspace's previous call on the device.
 *
 * Host buffers of any size: a kNN, k-th distance or radius-count call with
 * host queries or host outputs runs in batches of "host_batch" queries
 * (nbkd_set_tuning; default ~1 GiB of queries, results and unbudgeted device
 * scratch per batch) through two device slots and two pinned host staging
 * slots: the next batch's queries are copied in and the previous batch's
 * results copied out (DMA on a second stream, host copies on the library's
 * copy threads, "host_threads") while one batch computes, so device scratch
 * stays bounded for any m (the reference streams any m its host memory holds,
 * pybind.cpp:103-104,164-172).
 * Between batches the call runs the thread's interrupt check
 * (nbkd_set_interrupt; the reference polls PyErr_CheckSignals every 1000
 * queries, pybind.cpp:128-133) and returns NBKD_EINTR when it asks to stop.
 *
 * Every entry point returns an nbkd_status; on failure nbkd_last_error()
 * (thread-local) holds a message.  Statuses NBKD_EINVAL / NBKD_EBOX /
 * NBKD_ETOOMANY carry the reference's exact messages (kdtree/src/cpp/pybind.cpp:17,43-45,93;
 * kdtree/src/cpp/kdtree.cpp:99).
 */
#ifndef NBKD_H
#define NBKD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t nbkd_status;

enum {
    NBKD_OK = 0,
    NBKD_EINVAL = 1,   /* bad argument: shape, k <= 0, NULL pointer, ...              */
    NBKD_EBOX = 2,     /* periodic build: a coordinate outside [0, box_size]           */
    NBKD_ETOOMANY = 3, /* more than UINT32_MAX (padded) points                         */
    NBKD_ENOMEM = 4,   /* host or device allocation failed                             */
    NBKD_EDEVICE = 5,  /* HIP runtime error, no device, or kernel failure              */
    NBKD_EINTR = 6     /* the calling thread's interrupt check asked to stop (nbkd_set_interrupt) */
};

/* flags */
#define NBKD_INPUT_DEVICE 0x1u  /* point / query arrays are device pointers */
#define NBKD_OUTPUT_DEVICE 0x2u /* output arrays are device pointers        */
#define NBKD_ACCUMULATE 0x4u    /* nbkd_deposit: add into `out` instead of overwriting it */
#define NBKD_SQUARED 0x8u       /* nbkd_query_knn / _kth: output d2 (no sqrtf), the values
                                   the reference sorts by (kdtree.cpp:149-151) */
#define NBKD_SORTED 0x10u       /* nbkd_query_ball_csr: each row sorted ascending (on the device) */

typedef struct nbkd_tree nbkd_tree;

/* Node record, bit-identical to KDTree::KDTreeNode (kdtree/src/cpp/include/kdtree/kdtree.hpp:149-163). */
typedef struct {
    int32_t dimension; /* split axis, -1 = leaf                               */
    float split;       /* split value (internal nodes), 0.0f for leaves       */
    uint32_t left;     /* internal: left child id;  leaf: first point (tree order) */
    uint32_t right;    /* internal: right child id; leaf: one past the last point  */
} nbkd_node;

/*
 * Build a tree over n points given as an (n, 3) row-major float32 array.
 * Replaces: PyKDTree::PyKDTree / make_positions_and_indices (kdtree/src/cpp/pybind.cpp:14-56,76-88)
 *           and KDTree::KDTree (kdtree/src/cpp/kdtree.cpp:95-131).
 *   leaf_size  as the caller passes it; the reference clamps to >= 16
 *              (kdtree/src/cpp/include/kdtree/kdtree_impl.hpp:88-92).
 *   periodic   0 or 1; when 1 every coordinate must lie in [0, box_size].
 *   device     HIP device ordinal (< 0: the calling thread's current device).
 * The node table equals the reference's for the same (points, leaf_size):
 * preorder, left child = id + 1, split = the m-th order statistic with
 * m = (count/2)/8*8, leaves <= max(leaf_size, 16) points, padded to a multiple
 * of 8 with FLT_MAX coordinates and indices n..n8-1.
 */
nbkd_status nbkd_build(const float *xyz, uint64_t n, int32_t leaf_size, int32_t periodic,
                       float box_size, int32_t device, uint32_t flags, void *stream,
                       nbkd_tree **out);

/* NEW (slab trees): nbkd_build with extent = the points'
 * extent per axis (3 positive floats, host memory; NULL = nbkd_build).  Each
 * depth then splits the axis with the largest remaining extent (halved per
 * split, ties to the lower axis) instead of depth % 3, so a thin slab's
 * leaves are not flat: an x-slab of 1/8 of the box took 35 % more leaves
 * per query with depth % 3.  Same median rule, leaves and padding; the node
 * table differs from the reference's when the schedule does (extent (1, 1, 1)
 * gives depth % 3).  Query results: distances identical; indices identical up
 * to exact-distance ties (the traversal order differs, so which member of a
 * tied group a row holds may too). */
nbkd_status nbkd_build_ext(const float *xyz, uint64_t n, int32_t leaf_size, int32_t periodic,
                           float box_size, const float *extent, int32_t device, uint32_t flags,
                           void *stream, nbkd_tree **out);

/*
 * k nearest neighbours of m query points (row-major (m, 3) float32).
 * Replaces: PyKDTree::query (kdtree/src/cpp/pybind.cpp:90-189) and
 *           KDTree::find_closest (kdtree/src/cpp/kdtree.cpp:133-159).
 * out_dist / out_idx are (m, k) row-major: rows sorted by squared distance,
 * distances = sqrtf(d2); slots beyond the number of points hold
 * (sqrtf(FLT_MAX), 0xFFFFFFFF) as in the reference.
 */
nbkd_status nbkd_query_knn(const nbkd_tree *tree, const float *q, uint64_t m, int32_t k,
                           float *out_dist, uint32_t *out_idx, uint32_t flags, void *stream);

/*
 * Distance to the k-th nearest neighbour of each query (m floats): exactly
 * column k-1 of nbkd_query_knn's out_dist, without writing the (m, k) rows.
 * For local densities k / (4/3 pi r_k^3) and SPH-style smoothing lengths
 * (the per-point radii the reference's rasterizer consumes:
 * rasterization/src/python/nbodyhpc/rasterizer/__init__.py:104-143).
 * Replaces: row[k-1] of PyKDTree::query (pybind.cpp:90-189).  NEW.
 */
nbkd_status nbkd_query_kth(const nbkd_tree *tree, const float *q, uint64_t m, int32_t k,
                           float *out_dist, uint32_t flags, void *stream);

/*
 * NEW (no reference counterpart): number of points with d2 <= r*r of each
 * query (periodic metric when the tree is periodic).  out_count is (m,) uint32.
 * The radius contract, shared by nbkd_query_ball_csr, nbkd_query_ball_hist
 * and nbkd_fof (and, per edge, by nbkd_query_ball_sum, _profile and _hist2):
 * the threshold is T = min(fl(r*r), FLT_MAX), the product formed in float32,
 * and a point is inside iff d2 <= T in float32.
 *   - a negative r acts as |r|; r = 0 (and any r whose square underflows to
 *     0) reaches coincident points only;
 *   - r = NaN matches nothing (T is NaN);
 *   - r = +-inf, or any r whose square overflows (|r| >= 1.8447e19), reaches
 *     exactly the points whose d2 is finite;
 *   - padding points are in no ball for every r;
 *   - a query with a NaN coordinate has an empty ball (an empty row, all-zero
 *     bins), and so has a query whose d2 to every point overflows (an
 *     infinite coordinate, or one of about 1.8e19 and beyond).  Such a query
 *     changes nothing in the results of the other queries of the call.
 * The same queries in nbkd_query_knn and nbkd_query_kth give the reference's
 * row for a query that finds nothing: all (sqrtf(FLT_MAX), 0xFFFFFFFF), or
 * FLT_MAX with NBKD_SQUARED.
 * Out of scope (unspecified values, untested): non-finite point coordinates
 * at build time, and non-finite queries to nbkd_gravity and nbkd_group_*
 * (nbkd_gravity_ewald defines its own rule).
 */
nbkd_status nbkd_query_ball_count(const nbkd_tree *tree, const float *q, uint64_t m, float r,
                                  uint32_t *out_count, uint32_t flags, void *stream);

/*
 * NEW (no reference counterpart): the radius count for nr radii in one tree
 * walk: the pair counts DD(r) of a correlation function, cumulative neighbour
 * profiles, densities at several scales (scipy's count_neighbors(other, r)
 * with an array r).  radii is (nr,) float32, host memory, ascending (equal
 * neighbours allowed), each finite and >= 0, 1 <= nr <= NBKD_MAX_RADII.  The
 * count of query i at radius j is the number of points with d2 <= r[j]*r[j]
 * (float32, the tree's metric): column j of out_counts equals
 * nbkd_query_ball_count(q, r[j]) bit for bit, under that call's radius
 * contract: the threshold is min(fl(r[j]*r[j]), FLT_MAX), so a radius whose
 * square overflows counts the points at a finite d2 and never a padding
 * point, and a query with a NaN coordinate or with every d2 = inf has an
 * all-zero row.  Counts are cumulative in j; per-bin counts are their
 * differences.
 *   out_counts  (m, nr) row-major uint32, host or device memory
 *               (NBKD_OUTPUT_DEVICE), or NULL
 *   out_total   (nr,) uint64, always host memory, or NULL: the sum of column j
 *               over the m queries (exact: integer atomics on the device)
 * At least one of the two must be given.  With out_total the call returns when
 * both outputs are complete; with out_total == NULL and device queries and
 * counts it returns once the work is enqueued, as nbkd_query_ball_count does.
 * Host arrays stream in batches (see above); the totals accumulate over them.
 * m == 0 is NBKD_OK with out_total zeroed.
 */
#define NBKD_MAX_RADII 32
nbkd_status nbkd_query_ball_hist(const nbkd_tree *tree, const float *q, uint64_t m,
                                 const float *radii, int32_t nr, uint32_t *out_counts,
                                 uint64_t *out_total, uint32_t flags, void *stream);

/*
 * NEW (no reference counterpart): anisotropic pair counts in one tree walk:
 * every (query, point) pair classified on two coordinates about a line of
 * sight along one coordinate axis.  DD(rp, pi), from which the projected
 * correlation function wp(rp) is summed, and DD(s, mu), from which the
 * multipoles xi_0, xi_2, xi_4 are.  Cross counts and DR / RR come from passing
 * the other catalogue as the queries.
 *   q          (m, 3) float32, host or device (NBKD_INPUT_DEVICE)
 *   mode       NBKD_HIST2_RPPI or NBKD_HIST2_SMU
 *   los        0, 1 or 2: the axis of the line of sight
 *   edges1     (n1,) float32, host memory, ascending (equal neighbours allowed),
 *              each finite and >= 0, 1 <= n1 <= NBKD_MAX_RADII: rp or s edges
 *   edges2     (n2,) float32, host memory, under the same rules, 1 <= n2 <=
 *              NBKD_MAX_LOS_BINS: pi edges, or mu edges, each then also <= 1
 *   out_total  (n1, n2) row-major uint64, always host memory, required
 * Per-axis quantities, for query i and tree point j, per axis a, in float32
 * without fused multiply-adds: a_a = fl(d*d) with d = fl(p_a - q_a); on a
 * periodic tree the smallest of the three squares of d, fl(d - L), fl(d + L).
 * These are the terms the tree's d2 adds up; nothing here is a new metric.
 *   pi2 = a_los
 *   rp2 = fl(a_u + a_v), u < v the other two axes
 *   s2  = fl(fl(a_x + a_y) + a_z) whatever los is: the d2 of
 *         nbkd_query_ball_count, bit for bit
 * Thresholds, formed on the host in float32: T1[k] = fl(edges1[k] * edges1[k]);
 * RPPI: T2[l] = fl(edges2[l] * edges2[l]); SMU: M[l] = fl(edges2[l] * edges2[l]).
 * A product that overflows counts as FLT_MAX (nbkd_query_ball_sum's rule).
 * Bins, with the test written !(x <= t) as in nbkd_query_ball_hist:
 *   RPPI  b1 = #{k : !(rp2 <= T1[k])},  b2 = #{l : !(pi2 <= T2[l])}
 *   SMU   b1 = #{k : !(s2 <= T1[k])};  if b1 < n1,
 *         b2 = #{l : !(pi2 <= fl(M[l] * s2))}
 * The pair adds 1 to out_total[b1, b2] iff b1 < n1 and b2 < n2, otherwise
 * nowhere.  Bins are differential in both directions: a cumulative table
 * belongs to the caller.  Padding points are in no bin.
 * By monotone rounding pi2 <= s2 always, so with a last mu edge of exactly 1
 * every pair with b1 < n1 is counted, and the sum over b2 of row b1 equals the
 * first difference of nbkd_query_ball_hist's totals at edges1.  A pair with
 * s2 == 0 (the query itself, any coincident point) falls into bin (0, 0) in
 * both modes.  Untested: coordinates so small that M[l] * s2 is subnormal.
 * Counts are exact integers (integer atomics only, no floating-point
 * accumulation anywhere): the result does not depend on the leaf size, the
 * path (self order or bucketed), the host batch size, the grid or timing.
 * NBKD_EINVAL before any device call, out_total untouched, with a message
 * that names the function and the offending index: a NULL tree, q, edge array
 * or out_total; mode or los out of range; n1 or n2 out of range; an edge that
 * is NaN, infinite or negative, below its predecessor, or (mu) above 1;
 * m >= 2^32.  m == 0 is NBKD_OK with out_total zeroed.
 * The call returns when out_total is complete.  Host queries stream in batches
 * (see above) with no per-query output; the totals accumulate over the
 * batches and the thread's interrupt check runs between them.
 * Out of scope: there are no per-query rows, no pair weights and no jackknife
 * regions (a region's counts come from passing that region's points as the
 * queries).
 */
#define NBKD_HIST2_RPPI 0      /* first axis rp (perpendicular), second axis pi (along the line of sight) */
#define NBKD_HIST2_SMU  1      /* first axis s (= the tree's distance), second axis mu = pi / s */
#define NBKD_MAX_LOS_BINS 64   /* second axis; the first axis keeps NBKD_MAX_RADII = 32 */
nbkd_status nbkd_query_ball_hist2(const nbkd_tree *tree, const float *q, uint64_t m,
                                  int32_t mode, int32_t los,
                                  const float *edges1, int32_t n1,   /* host, ascending */
                                  const float *edges2, int32_t n2,   /* host, ascending */
                                  uint64_t *out_total,               /* (n1, n2) row-major, host */
                                  uint32_t flags, void *stream);

/*
 * NEW (no reference counterpart): nbkd_query_ball_hist2 in the observer frame,
 * for light cones, cut-sky mocks and survey catalogues with their randoms: the
 * line of sight of each pair runs from the observer through the pair's
 * midpoint (the convention of Corrfunc's DDrppi_mocks / DDsmu_mocks), not
 * along a coordinate axis.  DD, DR and RR for the Landy-Szalay estimator come
 * from passing the data or the randoms as the queries of the data's or the
 * randoms' tree.
 *   observer   (3,) float32, host memory, each component finite
 * The edges, the thresholds T1, T2 and M, the bin rule, the flags, the
 * streaming of host queries, the interrupt check, m == 0 and "returns when
 * out_total is complete" are those of nbkd_query_ball_hist2, word for word.
 * Only the two coordinates of a pair change.  All of it is float32 without
 * fused multiply-adds, every division IEEE correctly rounded (denormals
 * included).  For query i (position q), tree point j (position p), observer o,
 * per axis a:
 *   s_a  = fl(p_a - q_a)
 *   s2   = fl(fl(s_x*s_x + s_y*s_y) + s_z*s_z)     the d2 of nbkd_query_ball_count,
 *                                                  bit for bit
 *   l_a  = fl(fl(p_a - o_a) + fl(q_a - o_a))       twice the midpoint's offset from
 *                                                  the observer
 *   dot  = fl(fl(fl(s_x*l_x) + fl(s_y*l_y)) + fl(s_z*l_z))
 *   l2   = fl(fl(fl(l_x*l_x) + fl(l_y*l_y)) + fl(l_z*l_z))
 *   x    = fl(dot*dot)
 *   pi2  = l2 > 0 ? fminf(fl(x / l2), s2) : 0      the clamp makes pi2 <= s2 hold in
 *                                                  float32 (fminf: s2 where the
 *                                                  quotient is NaN)
 *   rp2  = fl(s2 - pi2)                            >= 0 by the clamp
 * Bins, with T1, T2 and M formed as in nbkd_query_ball_hist2:
 *   RPPI  b1 = #{k : !(rp2 <= T1[k])},  b2 = #{l : !(pi2 <= T2[l])}
 *   SMU   b1 = #{k : !(s2 <= T1[k])};  if b1 < n1,
 *         b2 = #{l : !(pi2 <= fl(M[l] * s2))}
 * The pair adds 1 to out_total[b1, b2] iff b1 < n1 and b2 < n2.  Consequences:
 *   - the ordered pairs (i, j) and (j, i) fall into the same bin: s negates
 *     exactly, l is a commutative sum, so dot negates exactly and x is
 *     unchanged.  Every bin of an auto count is therefore even once the n self
 *     pairs leave bin (0, 0);
 *   - a pair with s2 == 0 is in bin (0, 0);
 *   - with a last mu edge of exactly 1 every pair with b1 < n1 is counted, and
 *     the row sums equal the first difference of nbkd_query_ball_hist's totals
 *     at edges1;
 *   - l2 == 0 is defined as pi2 = 0: both points at the observer, or the two
 *     points mirror images about it;
 *   - padding points are in no bin;
 *   - a query with a NaN coordinate, or with every s2 infinite, is in no bin
 *     and changes nothing for the others;
 *   - x = fl(dot*dot) overflows once |s| |l| passes 2^64 (about 1.8e19): the
 *     quotient is then infinite and the clamp gives pi2 = s2, rp2 = 0.  Keep
 *     the product of the separation and the distance below that.
 * NBKD_EINVAL before any device call, out_total untouched, with a message that
 * names nbkd_query_ball_hist2_obs and the offending index: every condition of
 * nbkd_query_ball_hist2 except los; observer == NULL; an observer component
 * that is NaN or infinite.  After those checks (and after m == 0, which is
 * NBKD_OK with out_total zeroed) the handle is read: a periodic tree is
 * NBKD_EINVAL, pairwise lines of sight are defined for non-periodic trees only
 * (nbkd_query_ball_hist2 serves the periodic box).
 * Out of scope: pair weights, per-query rows, jackknife regions, periodic
 * trees, and other line-of-sight conventions (the bisector of the two
 * directions, the first point's direction).
 */
nbkd_status nbkd_query_ball_hist2_obs(const nbkd_tree *tree, const float *q, uint64_t m,
                                      int32_t mode,            /* NBKD_HIST2_RPPI | NBKD_HIST2_SMU */
                                      const float *observer,   /* (3,) host memory, finite */
                                      const float *edges1, int32_t n1,
                                      const float *edges2, int32_t n2,
                                      uint64_t *out_total,     /* (n1, n2) row-major, host */
                                      uint32_t flags, void *stream);

/*
 * NEW (no reference counterpart): friends-of-friends groups of the tree's own
 * points, the halo finder's first step.  Points i and j are friends iff
 * d2(i, j) <= b*b in float32, with d2 the tree's metric and b*b formed in
 * float32: exactly the predicate of nbkd_query_ball_count
 * (((dx^2 + dy^2) + dz^2), per-axis minimum image on a periodic tree).  Groups
 * are the connected components of the friendship graph; a point without a
 * friend is a group of one.  b == 0 is valid (only coincident points link); b
 * NaN, infinite or negative is NBKD_EINVAL.  The threshold follows
 * nbkd_query_ball_count's radius contract, min(fl(b*b), FLT_MAX): a finite b
 * whose square overflows links every pair of real points (one group) and no
 * padding point.
 *   out_label   (n,) uint32, required: out_label[i] = the smallest input row of
 *               i's group.  Labels are input rows 0..n-1 (the build's
 *               permutation), also after nbkd_set_ids replaced the ids.  The
 *               labelling is canonical: two calls give arrays equal under ==.
 *   out_size    (n,) uint32 or NULL: out_size[l] = the member count of the
 *               group whose label is l, 0 at every row that is not a label
 *               (sum = n, number of nonzeros = *out_ngroups).
 *   out_ngroups host memory, or NULL: the number of groups.
 * Padding points are in no group; no element >= n is written.
 * NBKD_OUTPUT_DEVICE: out_label and out_size are device pointers; with
 * out_ngroups == NULL the call then returns once the work is enqueued, as
 * nbkd_query_ball_count does, otherwise when every output is complete.
 * One tree walk with bound b*b over the points in tree order joins friends in
 * a lock-free union-find (integer atomics only).  Scratch: 8 bytes per point
 * of the call's workspace (two uint32 per tree position), plus staging of the
 * host outputs.
 */
nbkd_status nbkd_fof(const nbkd_tree *tree, float b, uint32_t *out_label, uint32_t *out_size,
                     uint64_t *out_ngroups, uint32_t flags, void *stream);

/*
 * NEW (no reference counterpart): kernel-weighted sums over each query's own
 * ball, the gather form of SPH (rho_i = sigma / h_i^3 * sum_j m_j K(d_ij / h_i))
 * and, with several value channels, field interpolation at arbitrary points.
 *   q          (m, 3) float32
 *   h          (m,) float32: query i's own radius, on the same side as q
 *              (both host, or both device with NBKD_INPUT_DEVICE)
 *   values     (n, nv) row-major float32 on the same side as q, indexed by input
 *              row (the build's permutation, also after nbkd_set_ids), or NULL:
 *              weight 1, nv must then be 1.  1 <= nv <= NBKD_MAX_VALUES.
 *   out_sum    (m, nv) float32 or NULL;  out_count (m,) uint32 or NULL; at least
 *              one; both host, or both device with NBKD_OUTPUT_DEVICE
 * Point j is a neighbour of query i iff d2(i, j) <= h_i*h_i in float32 (the
 * product formed in float32; a product that overflows counts as FLT_MAX):
 * nbkd_query_ball_count's predicate with r = h_i, so with every h_i = r
 * out_count equals nbkd_query_ball_count(q, r) bit for bit.
 * out_sum[i, c] = sum_j values[j, c] * K(u_ij), every step in float32 without
 * fused multiply-adds: inv_i = 1.0f / h_i (0 when h_i == 0),
 * u = fminf(sqrtf(d2) * inv_i, 1.0f), and
 *   NBKD_KERNEL_TOPHAT    K = 1
 *   NBKD_KERNEL_CUBIC     u <= 1/2: (1 - 6*(u*u)) + 6*((u*u)*u)
 *                         u >  1/2: w = 1 - u; 2*((w*w)*w)
 *   NBKD_KERNEL_WENDLAND  w = 1 - u; w2 = w*w; (w2*w2)*(1 + 4*u)
 * The sum is un-normalised: sigma / h^3 belongs to the caller (sigma = 3/(4 pi),
 * 8/pi, 21/(2 pi) for the three kernels).  A query whose h_i is NaN, infinite
 * or negative has an empty ball (sum 0, count 0); h_i == 0 reaches coincident
 * points only, with u = 0.
 * Deterministic: there are no floating-point atomics; each (query, channel) is
 * summed by one lane into one float32 accumulator in the tree's traversal
 * order (a periodic query outside [0, L]^3 by a fixed-order reduction over all
 * points), so two identical calls give arrays that are equal under ==.  A call
 * whose queries are the tree's build array (the self-order path) and one with
 * other queries may differ in the last bits of out_sum, never in out_count.
 * NBKD_EINVAL before any device call: NULL tree, q or h; both outputs NULL; nv
 * out of range; values == NULL with nv != 1; an unknown kernel; m >= 2^32.
 * m == 0 is NBKD_OK.  With device inputs and outputs the call returns once the
 * work is enqueued, as nbkd_query_ball_count does.  Host arrays stream in
 * batches (see above); values are uploaded once per call.  Scratch: 4 nv bytes
 * per point of the call's workspace (the values in tree order).
 */
#define NBKD_KERNEL_TOPHAT   0   /* K(u) = 1                                   */
#define NBKD_KERNEL_CUBIC    1   /* K(u) = 1 - 6u^2 + 6u^3 (u <= 1/2), 2(1-u)^3 */
#define NBKD_KERNEL_WENDLAND 2   /* K(u) = (1-u)^4 (1 + 4u)   (Wendland C2)     */
#define NBKD_MAX_VALUES 4
nbkd_status nbkd_query_ball_sum(const nbkd_tree *tree, const float *q, uint64_t m,
                                const float *h, const float *values, int32_t nv,
                                int32_t kernel, float *out_sum, uint32_t *out_count,
                                uint32_t flags, void *stream);

/*
 * NEW (no reference counterpart): weighted radial profiles around each query
 * in one tree walk: the mass (or any per-particle channel) in nr shells, with
 * the shell edges shared by all queries or in units of each query's own scale.
 * What spherical-overdensity masses and radii (M200c, R200c), stacked profiles
 * and concentrations are read from; with the tree's points as queries, the
 * weighted pair counts of a marked correlation function.
 *   q          (m, 3) float32
 *   scale      (m,) float32 on the same side as q (both host, or both device
 *              with NBKD_INPUT_DEVICE), or NULL
 *   radii      (nr,) float32, host memory, ascending (equal neighbours allowed),
 *              each finite and >= 0, 1 <= nr <= NBKD_MAX_RADII: the conditions
 *              of nbkd_query_ball_hist
 *   values     (n, nv) row-major float32 on the same side as q, indexed by input
 *              row (the build's permutation, also after nbkd_set_ids), or NULL:
 *              weight 1, nv must then be 1.  1 <= nv <= NBKD_MAX_VALUES.
 *   out_sum    (m, nr, nv) row-major float32, required; host, or device with
 *              NBKD_OUTPUT_DEVICE
 * Edges and thresholds of query i, in float32: e_ik = fl(radii[k] * scale[i]),
 * or radii[k] when scale == NULL; t_ik = fl(e_ik * e_ik), a product that
 * overflows counts as FLT_MAX (nbkd_query_ball_sum's rule).  Rounding is
 * monotone, so the t_ik are non-decreasing in k.  A query whose scale is NaN,
 * infinite or negative has an empty row (all zeros); scale 0 reaches coincident
 * points only (bin 0).
 * Point j falls into bin b = #{k : !(d2(i, j) <= t_ik)}, with d2 the tree's
 * float32 metric: the test of nbkd_query_ball_count.  b == nr means the point
 * is outside and added nowhere.  Padding points are in no bin.
 * out_sum[i, b, c] = sum_j values[j, c] over the points of bin b.  The result
 * is per-bin, not cumulative: a cumulative sum belongs to the caller, in
 * float64.  With values == NULL and scale == NULL the running sum over b of row
 * i (exact: integers below 2^24) equals row i of nbkd_query_ball_hist at the
 * same radii.
 * Deterministic: there are no floating-point atomics; each (i, b, c) is summed
 * by one lane into one float32 accumulator in the tree's traversal order (a
 * periodic query outside [0, L]^3 by a fixed-order reduction over all points),
 * without fused multiply-adds (there is no product), so two identical calls
 * give arrays that are equal under ==.  As with nbkd_query_ball_sum, a call
 * whose queries are the tree's build array (the self-order path), one with
 * other queries and other host batch sizes may differ in the last bits of a
 * sum, never in which points a bin holds.
 * NBKD_EINVAL before any device call, outputs untouched: NULL tree, q, radii or
 * out_sum; nr or nv out of range; values == NULL with nv != 1; radii not
 * ascending, not finite or negative; m >= 2^32.  m == 0 is NBKD_OK.  With
 * device inputs and outputs the call returns once the work is enqueued, as
 * nbkd_query_ball_sum does.  Host arrays stream in batches (see above), each
 * batch's slice of scale with its queries; values are uploaded once per call.
 * Scratch: 4 nv bytes per point of the call's workspace (the values in tree
 * order).
 */
nbkd_status nbkd_query_ball_profile(const nbkd_tree *tree, const float *q, uint64_t m,
                                    const float *scale,             /* (m,) or NULL          */
                                    const float *radii, int32_t nr, /* host, ascending       */
                                    const float *values, int32_t nv,
                                    float *out_sum,                 /* (m, nr, nv) row-major */
                                    uint32_t flags, void *stream);

/*
 * NEW (no reference counterpart): Barnes-Hut potentials and accelerations at
 * m query points from the tree's points as masses, G = 1 (the caller scales),
 * Plummer softening eps: what unbinding, the most-bound particle and a force
 * check of a snapshot need.
 *   q        (m, 3) float32
 *   mass     (n,) float32 on the same side as q, indexed by input row (the
 *            build's permutation, also after nbkd_set_ids), or NULL: mass 1.
 *            Masses must be finite and >= 0; otherwise the values are
 *            unspecified, but nothing faults.
 *   theta    the opening angle, 0 <= theta < 1; 0 is the direct sum
 *   eps      the softening length, finite and >= 0
 *   out_phi  (m,) float32 or NULL;  out_acc (m, 3) row-major float32 or NULL; at
 *            least one; both host, or both device with NBKD_OUTPUT_DEVICE
 * Non-periodic trees only: a periodic tree is NBKD_EINVAL (Ewald sums are not
 * provided).  nbkd_gravity_ewald below is the call for a periodic tree.
 * Everything below is float32 without fused multiply-adds unless float64 is
 * stated.
 * Node moments.  Each node with at least one real point has moments; padding
 * points are in no node's moments (no node is without a real point).
 *   M64 = sum m_j and S64 = sum m_j*p_j per axis, in float64, each product
 *   formed in float64 (exact: 24 x 24 bits); in a leaf by ascending tree
 *   position into one accumulator, in an internal node the left child's sums
 *   plus the right child's.  M = (float)M64; c = (float)(S64 / M64) per axis,
 *   the division in float64; if M64 == 0, c = 0.5f*(lo + hi) of the tight box.
 *   The tight box [lo, hi] is the exact min / max over the node's real points;
 *   e = hi - lo per axis; s2 = (e.x*e.x + e.y*e.y) + e.z*e.z.
 * Opening test, per query, at every node (leaves too): d = c - q per axis,
 * d2 = (d.x*d.x + d.y*d.y) + d.z*d.z; the node is accepted iff
 * theta*theta > 0 and s2 <= (theta*theta)*d2.  c lies inside the tight box and
 * theta < 1, so a query is never inside an accepted node's box.
 * Terms.  The walk starts at the root.  An accepted node adds the monopole
 * (M, c).  A leaf that is not accepted adds each of its real points (m_j, p_j)
 * with d = p_j - q, by ascending tree position.  An internal node that is not
 * accepted visits its left child, then its right child.
 * One term with mass mu at offset d (d2 as above): d2 == 0 adds nothing (a self
 * query, any coincident point, for every eps); otherwise
 *   r2 = d2 + eps*eps;  inv = 1.0f / sqrtf(r2);
 *   phi -= mu*inv;  w = mu*((inv*inv)*inv);
 *   acc.x += w*d.x;  acc.y += w*d.y;  acc.z += w*d.z.
 * phi and acc start at 0.
 * Deterministic: each query is summed by one lane into one float32 register per
 * component, in exactly this order.  The order depends on the tree, the query,
 * theta and eps only: not on the other queries of the call, the path (the
 * tree's build array as device queries takes the self-order path, other
 * queries are bucketed and sorted), the host batch size, the grid or timing.
 * There are no floating-point atomics.  Two calls give arrays equal under ==,
 * and so do the self-order path, the bucketed path and every host batch size.
 * A call with one output gives that output exactly as the call with both.
 * NBKD_EINVAL before any device call, outputs untouched: NULL tree or q; both
 * outputs NULL; theta NaN, negative or >= 1; eps NaN, negative or infinite;
 * m >= 2^32; a periodic tree.  m == 0 is NBKD_OK.  With device inputs and
 * outputs the call returns once the work is enqueued, as nbkd_query_ball_sum
 * does.  Host arrays stream in batches (see above); mass is uploaded once per
 * call.  Scratch: 4 bytes per point (the masses in tree order) and 100 bytes
 * per node (a 32-byte record M, c, s2 per node, the float64 sums, the tight
 * box, a done word) of the call's workspace; the moments are rebuilt per call
 * (one launch over the leaves, one per tree level above them).
 */
nbkd_status nbkd_gravity(const nbkd_tree *tree, const float *q, uint64_t m,
                         const float *mass, float theta, float eps,
                         float *out_phi, float *out_acc,
                         uint32_t flags, void *stream);

/*
 * NEW (no reference counterpart): nbkd_gravity on a periodic tree: Barnes-Hut
 * potentials and accelerations of the tree's points and all their periodic
 * images (box size L), G = 1.  Arguments, sides, flags and streaming are those
 * of nbkd_gravity; here a non-periodic tree is the one rejected.
 * Definition.  In units of the box, with x in [-1/2, 1/2]^3, the periodic
 * potential of a unit mass at offset x is -psi(x), with zero mean over the box:
 *   psi(x)       = sum_n erfc(a|x-n|)/|x-n|
 *                  + (1/pi) sum_{h != 0} exp(-pi^2 |h|^2/a^2)/|h|^2 * cos(2 pi h.x)
 *                  - pi/a^2
 *   -grad psi(x) = sum_n (x-n)/r^3 * [erfc(a r) + (2 a r/sqrt(pi)) exp(-a^2 r^2)]
 *                  + 2 sum_{h != 0} (h/|h|^2) exp(-pi^2 |h|^2/a^2) sin(2 pi h.x)
 * (r = |x-n|; n and h run over the integer triples; the value does not depend
 * on the splitting parameter a).  The corrections to the nearest image's
 * Newtonian term are
 *   C_phi(x) = psi(x) - 1/|x|,      C_a(x) = -grad psi(x) - x/|x|^3,
 * with C_phi(0) = -2.8372975 (the limit) and C_a(0) = 0.  C_phi is even in
 * every axis; component a of C_a is odd in axis a and even in the other two.
 * Table.  NBKD_EWALD_N = 64 intervals over [0, 1/2] per axis: 65^3 nodes
 * x = (i, j, k)/128 of 4 float32 each (C_phi, C_ax, C_ay, C_az), 4.39 MB, the
 * node index of x slowest.  It is computed on the host in float64 once per
 * process (first use; host threads, at most 16), in units of the box, so one
 * table serves every L, and uploaded once per device.  Each stored value is
 * within 2e-9 absolute of the converged sum before it is rounded to float32;
 * node (0, 0, 0) holds (-2.8372975f, 0, 0, 0), and component a is 0 on the
 * plane x_a = 0.  nbkd_ewald_table copies it out.
 * Everything below is float32 without fused multiply-adds unless float64 is
 * stated.  Per call, on the host: iL = 1.0f/L, sc = 128.0f*iL, iL2 = iL*iL.
 * Offset.  Per axis the raw d = p - q is replaced by the nearest image: the
 * one of d, fl(d - L), fl(d + L) with the smallest magnitude, ties to the
 * earlier in that order (nbkd_group_catalog's rule).  Then
 * d2 = (d.x*d.x + d.y*d.y) + d.z*d.z.
 * Node moments, the opening test and the order of the terms are exactly
 * nbkd_gravity's, with d the wrapped offset: moments in float64 per node (they
 * do not depend on periodicity); a node is accepted iff theta*theta > 0 and
 * s2 <= (theta*theta)*d2 with d the wrapped offset to c; the walk is
 * depth-first and left-first, an accepted node adds its monopole (M, c), a
 * leaf that is not accepted adds its real points by ascending tree position.
 * With theta < 1 an accepted node has s < |d| <= (sqrt(3)/2) L, so no image of
 * the query lies inside its box.
 * One term with mass mu at wrapped offset d: d2 == 0 adds nothing (the query
 * itself, a coincident point, for every eps).  The constant -2.8372975*m/L
 * that a particle's own images add to its potential is thereby left out (it
 * exerts no force); a caller who wants it adds it.  Otherwise first the
 * Newtonian part exactly as in nbkd_gravity (the Plummer softening eps acts on
 * this part only):
 *   r2 = d2 + eps*eps;  inv = 1.0f / sqrtf(r2);
 *   phi -= mu*inv;  w = mu*((inv*inv)*inv);
 *   acc.x += w*d.x;  acc.y += w*d.y;  acc.z += w*d.z;
 * then the correction, per axis a:
 *   t_a = fabsf(d_a)*sc;  i_a = min((int)t_a, 63);  f_a = t_a - (float)i_a;
 * each of the four channels is interpolated trilinearly between the eight
 * nodes (i_x + 0|1, i_y + 0|1, i_z + 0|1), every step as a + f*(b - a): along
 * x (four values), then along y (two), then along z; component a of C_a is
 * negated when d_a < 0; then
 *   phi = phi - (mu*iL)*C_phi;
 *   acc.x = acc.x + (mu*iL2)*C_ax;  likewise y and z.
 * phi and acc start at 0.  Over 20 000 sampled offsets the interpolation errs
 * by up to 1.2e-4/L per unit mass in the potential and 5.6e-4/L^2 in an
 * acceleration component (the tests hold it below 1.5e-4 and 7e-4).
 * Outside queries.  A query with a coordinate outside [0, L] or NaN takes no
 * part in the walk: its potential and its three acceleration components are
 * quiet NaNs.  A caller wraps such points into the box first.
 * Deterministic: each query is summed by one lane into one float32 register per
 * component, in exactly this order.  The order depends on the tree, the query,
 * theta and eps only: not on the other queries of the call, the path (the
 * tree's build array as device queries takes the self-order path, other
 * queries are bucketed and sorted), the host batch size, the grid or timing.
 * There are no floating-point atomics.  Two calls give arrays equal under ==,
 * and so do the self-order path, the bucketed path and every host batch size.
 * A call with one output gives that output exactly as the call with both.
 * NBKD_EINVAL before any device call, outputs untouched: NULL tree or q; both
 * outputs NULL; theta NaN, negative or >= 1; eps NaN, negative or infinite;
 * m >= 2^32; a tree that is not periodic (the message names nbkd_gravity).
 * m == 0 is NBKD_OK.  With device inputs and outputs the call returns once the
 * work is enqueued; host arrays stream in batches; mass is uploaded once per
 * call, all as in nbkd_gravity.  Scratch: nbkd_gravity's; the table lives per
 * device, outside the workspaces, for the life of the process.
 */
#define NBKD_EWALD_N 64
nbkd_status nbkd_gravity_ewald(const nbkd_tree *tree, const float *q, uint64_t m,
                               const float *mass, float theta, float eps,
                               float *out_phi, float *out_acc,
                               uint32_t flags, void *stream);

/*
 * The correction table of nbkd_gravity_ewald, copied to host memory:
 * (NBKD_EWALD_N + 1)^3 * 4 floats, [i][j][k][C_phi, C_ax, C_ay, C_az] for the
 * offset (i, j, k)/(2*NBKD_EWALD_N) in units of the box.  Needs no device (the
 * first call of a process computes the table).  NBKD_EINVAL if out is NULL or
 * capacity (in floats) is too small.
 */
nbkd_status nbkd_ewald_table(float *out, uint64_t capacity);

/*
 * NEW (no reference counterpart): the group catalogue of a labelling of the
 * tree's points, the halo finder's second step: which rows are in each group,
 * and the float64 moments from which mass, centre, extent, bulk velocity and
 * velocity dispersion follow.
 *   label       (n,) uint32 by input row (the build's permutation, also after
 *               nbkd_set_ids), canonical: label[i] < n and
 *               label[label[i]] == label[i].  The output of nbkd_fof is; any
 *               canonical labelling is accepted.  A device kernel counts the
 *               violations: a nonzero count is NBKD_EINVAL with a message, and
 *               nothing is written but the two counts, which are zeroed.
 *   weight      (n,) float32, or NULL: weight 1
 *   values      (n, nv) row-major float32, or NULL with nv == 0;
 *               0 <= nv <= NBKD_MAX_VALUES
 *               label, weight and values are on one side: host, or device with
 *               NBKD_INPUT_DEVICE
 *   min_members a group is kept when it has at least this many members (0 is
 *               treated as 1).  Kept groups are numbered g = 0..G-1 by ascending
 *               label (the group's "head": its smallest row).
 *   out_ngroups, out_nmembers   host memory, required: G, and K = the number of
 *               rows in kept groups.  They are always written.
 *   group_capacity, member_capacity   if G > group_capacity or
 *               K > member_capacity no other output is written and the status
 *               is NBKD_OK: a sizing call is a call with both capacities 0, as
 *               with nbkd_query_ball_csr.
 * The other outputs are host memory, or device memory with NBKD_OUTPUT_DEVICE;
 * each may be NULL:
 *   out_head    (G,) uint32   the head of group g
 *   out_size    (G,) uint32   its member count
 *   out_offsets (G+1,) uint64 and
 *   out_members (K,) uint32   out_members[out_offsets[g] : out_offsets[g+1]] =
 *               the input rows of group g, ascending
 *   out_dmax    (G,) float32  the maximum over members and axes of |d| (exact:
 *               a maximum does not depend on the order).  On a periodic tree
 *               dmax >= L/2 means the group spans the box and the unwrapping
 *               relative to the head is not trustworthy.
 *   out_moments (G, NBKD_GROUP_MOMENTS(nv)) row-major float64; row g holds, over
 *               the members j of g,
 *                 [sum w, sum w*dx, sum w*dy, sum w*dz,
 *                  sum w*((dx*dx + dy*dy) + dz*dz),
 *                  sum w*v_c (c < nv), sum w*(v_c*v_c) (c < nv)]
 * d is the float32 offset of member j from the head's position: per axis
 * d = fl(p_j - p_head), and on a periodic tree the one of d, fl(d - L),
 * fl(d + L) with the smallest magnitude (ties to the earlier in that order).
 * Each term is formed in float64 from the float32 inputs exactly as written,
 * without fused multiply-adds (w*d is exact: 24 x 24 bits).
 * Deterministic: there are no floating-point atomics, and the summation order
 * is a fixed function of the sorted member list (64 consecutive members per
 * wave, a log-step segmented scan over the lanes, then a fixed-shape sum of
 * the per-wave partials of each group that crosses a wave).  It does not
 * depend on the tree, its leaf size, the launch geometry or timing: two calls
 * with the same labels, weights and values give moments equal under ==, also
 * across trees built from the same points with different leaf_size.
 * Any order of summing m float64 terms t_i errs by at most
 * (m - 1) * 2^-53 * sum |t_i|.
 * NBKD_EINVAL before any device call, outputs untouched: NULL tree, label,
 * out_ngroups or out_nmembers; nv out of range; values == NULL with nv != 0;
 * values != NULL with nv == 0.  n == 0 is NBKD_OK with both counts 0.  Padding
 * points are in no group.  The call always waits (the counts are host memory).
 * Scratch: 12 bytes per point (counts and two scans; one of them later holds
 * row -> tree position), 16 bytes per kept row (the radix sort's two key /
 * row pairs), 2 * NBKD_GROUP_MOMENTS(nv) * 8 + 12 bytes per 64 kept rows (the
 * per-wave partials), the uploaded host inputs and the staged host outputs.
 */
#define NBKD_GROUP_MOMENTS(nv) (5 + 2 * (nv))
nbkd_status nbkd_group_catalog(const nbkd_tree *tree, const uint32_t *label,
                               const float *weight, const float *values, int32_t nv,
                               uint32_t min_members,
                               uint64_t group_capacity, uint64_t member_capacity,
                               uint64_t *out_ngroups, uint64_t *out_nmembers,
                               uint32_t *out_head, uint32_t *out_size,
                               uint64_t *out_offsets, uint32_t *out_members,
                               double *out_moments, float *out_dmax,
                               uint32_t flags, void *stream);

/*
 * NEW (no reference counterpart): per-group potentials, the halo finder's
 * third step: for every entry of a list of row groups the potential of its own
 * group's other entries at its position (what unbinding needs), and per group
 * the entry of lowest potential (the most-bound particle, the usual halo
 * centre).  A segmented direct sum, one call for all groups; G = 1.
 *   offsets   (ngroups+1,) uint64 and
 *   members   (nmembers,) uint32: members[offsets[g] : offsets[g+1]] = the input
 *             rows of group g, as nbkd_group_catalog writes them.  Any grouping
 *             is accepted: the groups need not be FoF groups, rows may be
 *             missing and rows may repeat, so a list trimmed by the caller (a
 *             round of unbinding) goes straight back in.
 *   mass      (n,) float32 by input row (the build's permutation, also after
 *             nbkd_set_ids), or NULL: mass 1.  Masses must be finite and >= 0;
 *             otherwise the values are unspecified, but nothing faults.
 *             offsets, members and mass are on one side: host, or device with
 *             NBKD_INPUT_DEVICE
 *   eps       the softening length, finite and >= 0
 *   max_members  0: no limit.  Otherwise a group with more than max_members
 *             entries is skipped: its out_phi entries are quiet NaNs and its
 *             out_minpos is 0xFFFFFFFF.  The work is the sum over the groups of
 *             s*s terms (s = the group's entry count): one group of 1e6 entries
 *             is 1e12 terms.  Callers who cannot bound s should set max_members.
 *   out_phi   (nmembers,) float32, aligned with members, or NULL
 *   out_minpos (ngroups,) uint32, or NULL; at least one of the two; both host
 *             memory, or both device memory with NBKD_OUTPUT_DEVICE
 * Definition.  Entry e lies in group g when offsets[g] <= e < offsets[g+1];
 * i = members[e].  Everything is float32 without fused multiply-adds unless
 * float64 is stated.  acc64 = 0.0; for f = offsets[g] .. offsets[g+1]-1 in
 * ascending order, j = members[f]:
 *   d2 = the tree's metric between p_i and p_j (the kNN metric): d = p_j - p_i
 *        per axis, on a periodic tree the minimum over |d|, |d - L|, |d + L|
 *        per axis, then d2 = (d.x*d.x + d.y*d.y) + d.z*d.z;
 *   d2 == 0 adds nothing (the entry itself, a repeated row, any coincident
 *        point, for every eps); otherwise
 *   r2 = d2 + eps*eps;  inv = 1.0f / sqrtf(r2);  acc64 += (double)(m_j*inv).
 * out_phi[e] = (float)(-acc64).
 * This is the isolated potential of the group under the minimum image.  On a
 * periodic tree it is meaningful for groups with dmax < L/2 (nbkd_group_catalog's
 * out_dmax: the group does not span the box); no Ewald sum is involved.
 * out_minpos[g] = the smallest e of group g with the lowest out_phi[e], compared
 * as the float32 values written (-0 and +0 are equal), so an argmin over
 * out_phi[offsets[g] : offsets[g+1]] on the host gives the same entry; its row
 * is members[out_minpos[g]].  Empty groups and skipped groups get 0xFFFFFFFF.
 * Deterministic: one lane sums one entry into one float64 accumulator in list
 * order; there are no floating-point atomics (the minimum is a 64-bit integer
 * atomic over an order-preserving key, which commutes).  The result depends on
 * the points, the masses, the list and eps only: not on the tree's leaf size,
 * the launch geometry or timing.  Two calls give arrays equal under ==, and so
 * do trees built from the same points with different leaf_size.
 * NBKD_EINVAL before any device call, outputs untouched: NULL tree, offsets or
 * members; both outputs NULL; eps NaN, negative or infinite; ngroups or
 * nmembers >= 2^32.  ngroups == 0 is NBKD_OK and writes nothing; nmembers == 0
 * is NBKD_OK: every group is empty, out_minpos is all 0xFFFFFFFF.  Otherwise a
 * device kernel counts the violations of offsets[0] == 0, offsets
 * non-decreasing, offsets[ngroups] == nmembers and members[e] < n before
 * anything else runs: a nonzero count is NBKD_EINVAL with a message that gives
 * the count, and no output is written; no kernel indexes with an unchecked row
 * or offset.  The call always waits (the violation count is read on the host,
 * as in nbkd_group_catalog).
 * Scratch: 16 bytes per entry (x, y, z, m packed in list order), 4 bytes per
 * entry (the entry's group number), 4 bytes per point (row -> tree position),
 * 8 bytes per group (the argmin key), the uploaded host inputs and the staged
 * host outputs (4 bytes per entry also when out_phi is NULL).
 */
nbkd_status nbkd_group_potential(const nbkd_tree *tree,
                                 const uint64_t *offsets, const uint32_t *members,
                                 uint64_t ngroups, uint64_t nmembers,
                                 const float *mass, float eps, uint32_t max_members,
                                 float *out_phi, uint32_t *out_minpos,
                                 uint32_t flags, void *stream);

/*
 * NEW: neighbour lists within r in CSR form.  out_offsets is (m+1,) uint64
 * (always host memory); out_idx receives offsets[m] original point indices,
 * each row in tree traversal order, or ascending with NBKD_SORTED (a per-row
 * sort on the device).  Call with out_idx == NULL first to get offsets[m]
 * (the required capacity), then again with a buffer of that size.
 * The rows follow nbkd_query_ball_count's radius contract, and the counting
 * pass and the fill see the same threshold min(fl(r*r), FLT_MAX): row i holds
 * offsets[i + 1] - offsets[i] ids, each < n, for every r -- every point at a
 * finite d2 when r*r overflows (r = inf included), none for r = NaN or for a
 * query with a NaN coordinate.
 * Batched (round 6): the counts stream through the host-buffer pipeline; the
 * fill runs in batches of at most ~64 M ids (a row longer than that is a batch
 * of its own) whose ids are sorted and copied out while the next batch is
 * computed, so device scratch is bounded by the batch, not by m or offsets[m]
 * (the reference streams any m its host memory holds, pybind.cpp:103-104,164-172).
 * Queries and out_idx may be host or device memory (NBKD_INPUT_DEVICE /
 * NBKD_OUTPUT_DEVICE); the call returns when out_idx is complete.  Between
 * batches it runs the thread's interrupt check.
 */
nbkd_status nbkd_query_ball_csr(const nbkd_tree *tree, const float *q, uint64_t m, float r,
                                uint64_t *out_offsets, uint32_t *out_idx, uint64_t capacity,
                                uint32_t flags, void *stream);

/* n8 = padded point count (the reference's `n`), nodes = node count (`size`). */
nbkd_status nbkd_tree_info(const nbkd_tree *tree, uint64_t *n8, uint64_t *nodes,
                           int32_t *periodic, float *box_size, int32_t *device);

/* Copy the node table (nodes entries) and the tree-ordered SoA points and
 * original indices (n8 entries each) to host buffers; any may be NULL. */
nbkd_status nbkd_export(const nbkd_tree *tree, nbkd_node *nodes, float *x, float *y, float *z,
                        uint32_t *idx);

void nbkd_free(nbkd_tree *tree);

/* Process-wide tuning knobs (the library reads no environment variable):
 *   "knn_seed_margin"  a in the seed ball's expected count mu = k + a sqrt(k) + a
 *                      (default 3.0; > 0).  Results never depend on it: a query
 *                      whose seed ball holds fewer than k points is re-walked.
 *   "candidate_bytes"  HBM budget of one collect / select batch's candidate
 *                      columns (default 0 = min(96 GiB, free / 3)).
 *   "host_batch"       queries per batch of a host-buffer call (default 0 =
 *                      about 1 GiB of queries plus results per batch).
 *   "host_threads"     threads copying between the caller's host arrays and
 *                      pinned staging (default 0 = the usable cores, <= 16).
 *   "self_order"       1 (default): a kNN / k-th query whose queries are the
 *                      first m rows of the device array the tree was built from
 *                      (same pointer, NBKD_INPUT_DEVICE) runs in tree order
 *                      instead of bucketing and sorting the queries; 0: always
 *                      bucket and sort.  Results never depend on it (the order
 *                      and the seeds only steer the work).
 *   "pinned_bytes"     process-wide cap on the host-buffer pipeline's pinned
 *                      staging (default 0 = 8 GiB).  A call whose staging would
 *                      pass it, or whose hipHostMalloc fails, streams between
 *                      the caller's pageable arrays and the device instead
 *                      (same results, lower rate).  Idle workspaces release
 *                      their staging when a device allocation needs memory.
 *   "collect_wide_addr" 0 (default): the kNN collect kernel's tree walk loads
 *                      node records and cell boxes at 32-bit byte offsets from
 *                      the table bases wherever every offset fits (fewer than
 *                      2^27 nodes); 1: always through 64-bit addresses, the
 *                      instance larger trees take.  Results never depend on it.
 *   "collect_one_chunk" 1 (default): a tree with leaf size <= 64 takes the
 *                      collect kernel's one-chunk instance (no chunk loop, no
 *                      half-leaf boxes, staging loads at 32-bit offsets where
 *                      they fit); 0: the general instance that larger leaves
 *                      take.  Results never depend on it.
 *   "hist2_flush_visits" 0 (default): a wave of nbkd_query_ball_hist2 adds its
 *                      LDS histogram to the device totals at the end of its
 *                      packet and before a 32-bit word could wrap; v > 0: also
 *                      after every v leaf visits.  Results never depend on it.
 *   "hist2_copies"     0 (default = 2): the interleaved LDS copies of that
 *                      histogram per wave, rounded down to a power of two and
 *                      to what 8 KiB holds.  Results never depend on it.
 * NEW (no reference counterpart: kdtree/src/cpp/pybind.cpp:196-216 has no knobs). */
nbkd_status nbkd_set_tuning(const char *name, double value);
nbkd_status nbkd_get_tuning(const char *name, double *value);
/* 1 if a tree of `nodes` nodes takes the collect kernel's wide-address
 * instance under the current "collect_wide_addr" setting, else 0.  NEW. */
int32_t nbkd_collect_wide_addr(uint64_t nodes);
/* The kNN collect kernel's instance for a tree of `points` points and `nodes`
 * nodes built with `leaf_size`, under the current knobs: bit 0 set = the
 * one-chunk instance (leaf size <= 64: every leaf is staged whole, once);
 * bit 1 set = 32-bit byte offsets (the walk's, and for the one-chunk
 * instance also its staging loads': points * 16, points / 8 * 24 and
 * nodes * 32 must all be below 2^32).  NEW. */
int32_t nbkd_collect_instance(int32_t leaf_size, uint64_t points, uint64_t nodes);
/* Those three staging bounds one by one: bit 0 set = the point offsets fit
 * (points padded to a multiple of 8, times 16 B), bit 1 = the group-box
 * offsets (24 B per 8 points), bit 2 = the leaf-box offsets (32 B per node).
 * NEW. */
int32_t nbkd_collect_stage_offsets(uint64_t points, uint64_t nodes);

/* The calling thread's interrupt check: host-buffer query calls (kNN, k-th
 * distance, radius count) call fn(user) between batches and stop with
 * NBKD_EINTR when it returns nonzero (results of that call are then
 * undefined).  NULL removes it.  Replaces the reference's
 * PyErr_CheckSignals poll (kdtree/src/cpp/pybind.cpp:128-133).  NEW. */
typedef int (*nbkd_interrupt_fn)(void *user);
nbkd_status nbkd_set_interrupt(nbkd_interrupt_fn fn, void *user);

/* thread-local message of the last failure on this thread ("" if none) */
const char *nbkd_last_error(void);

/* number of visible HIP devices (0 and NBKD_OK when there are none) */
nbkd_status nbkd_device_count(int32_t *count);

/* Kernel timing with HIP events recorded on the launch stream.  While enabled,
 * each launch of a named kernel is bracketed by events; nbkd_timing_read
 * synchronises them and returns the summed milliseconds and launch count of
 * every launch of `name` since the last reset. */
nbkd_status nbkd_timing_enable(int32_t enable);
nbkd_status nbkd_timing_reset(void);
nbkd_status nbkd_timing_read(const char *name, double *ms, uint64_t *launches);

/* per-query work counters of the last kNN call on this thread (debug builds of
 * the statistics, KDTreeQueryStatistics kdtree/src/cpp/include/kdtree/kdtree.hpp:124-131):
 * sums over all queries of nodes visited and points scanned by the packet
 * traversal.  Enabled with nbkd_stats_enable(1); costs a few % when on. */
nbkd_status nbkd_stats_enable(int32_t enable);
nbkd_status nbkd_stats_read(uint64_t *nodes_visited, uint64_t *points_scanned);
/* all counters of the last kNN call: [0] nodes entered x packet lanes,
 * [1] (query, point) distance evaluations, [2] dense leaf rounds, [3] sparse
 * (lane-compacted) iterations, [4] top-k merges, [5] packets (waves),
 * [6] candidates merged (all lanes), [7] merges while some lane was still filling */
nbkd_status nbkd_stats_read_all(uint64_t *out, int32_t n);

/* ------------------------------------------------------------------ slabs (multi-GPU)
 * NEW (the reference is single-node CPU only).  One process per
 * GPU; the particles are cut into x-slabs [lo, hi) of the periodic box and each
 * rank builds its tree over its own particles plus halo strips of width h
 * received from its two ring neighbours.  All pointers here are device
 * pointers on `device`; xyz arrays are (n, 3) row-major float32. */

/* Replace the tree's point ids: idx[j] <- ids[idx[j]] for the n real points
 * (ids has n entries; host memory unless NBKD_INPUT_DEVICE).  kNN and ball
 * queries then return these ids (e.g. global particle ids of a slab tree). */
nbkd_status nbkd_set_ids(nbkd_tree *tree, const uint32_t *ids, uint32_t flags, void *stream);

/* A device array of `capacity` floats beside the tree's kNN rows: each later
 * nbkd_query_knn of the tree's own points (the first m <= capacity rows of
 * the device array it was built from) with NBKD_OUTPUT_DEVICE also writes
 * every row's last column (its k-th distance, as the row holds it) to
 * kth[row].  A slab's exactness test then reads 4 B per row instead of a
 * row's last line (nbkd_slab_forward_async with dist = kth, k = 1).  kth =
 * NULL or capacity = 0 detaches it; other calls leave it untouched.  The call
 * waits for every kNN of the tree already enqueued (on any stream), so the
 * previously attached array may be freed once it returns. */
nbkd_status nbkd_set_kth_out(nbkd_tree *tree, float *kth, uint64_t capacity);

/* Stable compaction of the points with lo <= x < hi into out_xyz / out_ids
 * (ids may be NULL: then the row number is stored).  *count receives the
 * number selected; with out_xyz or out_ids NULL only the count is computed. */
nbkd_status nbkd_slab_select(const float *xyz, const uint32_t *ids, uint64_t n, float lo, float hi,
                             float *out_xyz, uint32_t *out_ids, uint64_t capacity,
                             uint64_t *count, int32_t device, void *stream);

/* Exactness check of a slab-local kNN result: counts the queries (x in
 * [lo, hi)) whose k-th distance (column k-1 of the (m, k) dist rows) is not
 * strictly inside the local domain [lo - h, hi + h) along x.  Zero means every
 * row equals the single-tree result over all particles. */
nbkd_status nbkd_slab_violations(const float *q, const float *dist, uint64_t m, int32_t k,
                                 float lo, float hi, float h, uint64_t *count, int32_t device,
                                 void *stream);

/* Second-round exchange of a slab-local kNN result: the
 * own queries whose k-th distance (column k-1 of the (m, k) rows `dist`, or
 * the m distances with k = 1) reaches past the left face cl or the right face
 * ch of the covered x-range: bit 0 of out_sides = left, bit 1 = right (the
 * same f32 test as nbkd_slab_violations, split by side).  Up to `capacity`
 * query indices go to out_list (in no particular order); *count receives the
 * total, which may exceed the capacity (call again with a larger buffer). */
nbkd_status nbkd_slab_forward(const float *q, const float *dist, uint64_t m, int32_t k, float cl,
                              float ch, uint32_t *out_list, uint8_t *out_sides, uint64_t capacity,
                              uint64_t *count, int32_t device, void *stream);

/* nbkd_slab_forward without waiting: `count` is a device word (8 B) that the
 * call zeroes and the kernel fills on `stream`; nothing is read back, so a
 * caller can queue its next work before it copies the count out (the bench's
 * N > 1 step overlaps the second round's agreement with the next step). */
nbkd_status nbkd_slab_forward_async(const float *q, const float *dist, uint64_t m, int32_t k,
                                    float cl, float ch, uint32_t *out_list, uint8_t *out_sides,
                                    uint64_t capacity, uint64_t *count, int32_t device,
                                    void *stream);

/* Row gather / scatter of device arrays: dst[i] = src[idx[i]] (gather) or
 * dst[idx[i]] = src[i] (scatter) for n rows of row_bytes (a multiple of 4)
 * bytes; idx is a device array of uint32 row numbers. */
nbkd_status nbkd_rows_gather(const void *src, uint64_t row_bytes, const uint32_t *idx, uint64_t n,
                             void *dst, int32_t device, void *stream);
nbkd_status nbkd_rows_scatter(const void *src, uint64_t row_bytes, const uint32_t *idx, uint64_t n,
                              void *dst, int32_t device, void *stream);

/* RCCL communicator (librccl.so.1 loaded on first use).  Rank 0 calls
 * nbkd_comm_unique_id and distributes the NBKD_COMM_ID_BYTES bytes out of band
 * (e.g. torch.distributed over gloo); every rank then calls nbkd_comm_init. */
#define NBKD_COMM_ID_BYTES 128
typedef struct nbkd_comm nbkd_comm;
nbkd_status nbkd_comm_unique_id(uint8_t *out);
/* NBKD_OK iff librccl.so.1 loads with every symbol the exchange uses; unlike
 * nbkd_comm_unique_id it starts no bootstrap listener (every rank may call it). */
nbkd_status nbkd_comm_probe(void);
nbkd_status nbkd_comm_init(const uint8_t *id, int32_t rank, int32_t world, int32_t device,
                           nbkd_comm **out);
/* One grouped set of point-to-point byte transfers: for each i, send
 * send_bytes[i] from send[i] to rank send_peer[i] and receive recv_bytes[i]
 * into recv[i] from rank recv_peer[i] (zero sizes skip).  Transfers between
 * one pair of ranks are matched in posting order.  Enqueued on `stream`. */
nbkd_status nbkd_comm_exchange(nbkd_comm *comm, int32_t npairs, const void *const *send,
                               const uint64_t *send_bytes, const int32_t *send_peer,
                               void *const *recv, const uint64_t *recv_bytes,
                               const int32_t *recv_peer, void *stream);
void nbkd_comm_free(nbkd_comm *comm);

/*
 * Deposit n spheres (centres xyz row-major (n, 3), weight[n], radius[n]) onto a
 * voxel grid, with the semantics of the reference's point rasteriser:
 * replaces PointRenderer::render_points_volume / render_points
 * (rasterization/src/cpp/point_renderer.cpp:606-657,825-950), assemble_vertices
 * (rasterization/src/cpp/pybind.cpp:25-71), augment_vertices_periodic
 * (rasterization/src/cpp/vertex_utilities.cpp:15-42) and the vertex / fragment
 * shaders (rasterization/shaders/triangle.vert, triangle.frag).
 *   out        gx * gy * nz float32, element (px, py, s) at px + gx * (py + gy * s)
 *              (the reference's column-major (gx, gy, nz) array); zeroed first
 *              unless NBKD_ACCUMULATE is set.
 *   pixels_per_unit  voxels per unit length (> 0).
 *   period     3 floats (NULL = none); period[d] > 0 wraps axis d with that length.
 *   subsample  S: each straddled voxel is sampled at S^3 points (1..16).
 *   mode       0: nz slices [s, s+1) / ppu (render_points_volume);
 *              1: one plane at z = 0 (render_points; nz must be 1).
 *   x0, wx     `out` holds only the columns [x0, x0 + wx) of the gx-wide grid,
 *              element (px, py, s) at (px - x0) + wx * (py + gy * s); sprites,
 *              periodic images and clipping are those of the whole grid
 *              (0, gx: the whole grid).  One rank's x-slab (nbodyhpc_amd/slab.py).
 * A voxel receives weight * (sub-samples inside the ball) / S^3 / (4/3 pi R^3)
 * (R the radius in voxels); a ball under half a voxel across deposits its whole
 * weight in the voxel holding its centre.
 */
nbkd_status nbkd_deposit(const float *xyz, const float *weight, const float *radius, uint64_t n,
                         int32_t gx, int32_t gy, int32_t nz, float pixels_per_unit,
                         const float *period, int32_t subsample, int32_t mode, int32_t x0,
                         int32_t wx, float *out, int32_t device, uint32_t flags, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* NBKD_H */
