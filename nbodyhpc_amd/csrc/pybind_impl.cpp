// nbodyhpc_amd.kdtree._impl — pybind11 mirror of the reference binding
// kdtree/src/cpp/pybind.cpp:60-216 over the C ABI (include/nbkd.h).
//
// Same class name, constructor / method signatures and defaults
// (KDTree(points, leafsize=64, max_threads=-1, boxsize=None); query(points,
// k=1, workers=1)), same properties (n = padded count, size = node count,
// periodic, boxsize) and the same RuntimeError messages.  Differences, all
// additive: a trailing `device` constructor argument, radius queries
// (query_ball_count / query_ball_csr / query_ball_hist / query_ball_hist2 /
// query_ball_hist2_obs),
// kernel-weighted sums (ball_sum), radial profiles (ball_profile), gravity,
// gravity_ewald, fof_labels, group_moments, group_potential and export() for
// parity tests.
// `max_threads` and `workers` are accepted and ignored: the build and the
// queries run on the GPU (the reference ignores max_threads too,
// kdtree/src/cpp/kdtree.cpp:116).  Queries release the GIL, may be called from
// several Python threads on one tree at once (the library gives each call its
// own scratch), accept any number of rows (host buffers stream through bounded
// device memory) and stop with KeyboardInterrupt on Ctrl-C: the library polls
// PyErr_CheckSignals between batches, as the reference does every 1000 queries
// (kdtree/src/cpp/pybind.cpp:128-133).
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <new>
#include <optional>
#include <stdexcept>
#include <string>

#include "../../include/nbkd.h"

namespace py = pybind11;

namespace {

using farray = py::array_t<float, py::array::c_style | py::array::forcecast>;

[[noreturn]] void raise(nbkd_status st) {
    if (st == NBKD_ENOMEM) throw std::bad_alloc();
    throw std::runtime_error(nbkd_last_error());
}

// nbkd_set_interrupt callback: runs on the calling thread between batches of a
// host-buffer query, with the GIL released around it
int check_signals(void *hit) {
    py::gil_scoped_acquire gil;
    if (PyErr_CheckSignals() != 0) { // pybind.cpp:128-133
        *static_cast<bool *>(hit) = true;
        return 1;
    }
    return 0;
}

// one query call: the interrupt check installed for its duration (GIL held
// when constructed and when finish() runs)
struct Interruptible {
    bool hit = false;
    Interruptible() { nbkd_set_interrupt(check_signals, &hit); }
    ~Interruptible() { nbkd_set_interrupt(nullptr, nullptr); }
    void finish(nbkd_status st) {
        if (st == NBKD_EINTR && hit) throw py::error_already_set(); // KeyboardInterrupt
        if (st != NBKD_OK) raise(st);
    }
};

void check(nbkd_status st) {
    if (st != NBKD_OK) raise(st);
}

void check_shape(const farray &points) {
    if (points.ndim() != 2 || points.shape(1) != 3)
        throw std::runtime_error("positions must be a 2D array of shape (N, 3)"); // pybind.cpp:17,97
}

class PyKDTree {
    nbkd_tree *h_ = nullptr;
    bool periodic_ = false;
    float box_ = 0.0f;
    int device_ = 0;
    uint64_t n8_ = 0, nodes_ = 0;
    uint64_t n_in_ = 0; // the caller's point count (n8_ is the padded one)

  public:
    PyKDTree(farray points, int leaf_size, int /*max_threads*/, std::optional<float> box_size,
             int device) {
        check_shape(points);
        periodic_ = box_size.has_value();
        box_ = box_size.value_or(0.0f);
        const float *ptr = points.data();
        const uint64_t n = (uint64_t)points.shape(0);
        nbkd_status st;
        {
            py::gil_scoped_release nogil; // pybind.cpp:86
            st = nbkd_build(ptr, n, leaf_size, periodic_ ? 1 : 0, box_, device, 0u, nullptr, &h_);
        }
        check(st);
        n_in_ = n;
        int32_t dev = 0;
        check(nbkd_tree_info(h_, &n8_, &nodes_, nullptr, nullptr, &dev));
        device_ = dev;
    }
    PyKDTree(const PyKDTree &) = delete;
    PyKDTree &operator=(const PyKDTree &) = delete;
    ~PyKDTree() {
        if (h_) nbkd_free(h_);
    }

    size_t num_points() const { return (size_t)n8_; }
    size_t num_nodes() const { return (size_t)nodes_; }
    bool periodic() const { return periodic_; }
    float box_size() const { return box_; }
    int device() const { return device_; }

    // pybind.cpp:90-189
    std::pair<py::array_t<float>, py::array_t<uint32_t>> query(farray points, int k, int workers) {
        (void)workers;
        if (k <= 0) throw std::runtime_error("k must be positive integer");
        check_shape(points);
        const py::ssize_t m = points.shape(0);
        py::array_t<float> dist({m, (py::ssize_t)k});
        py::array_t<uint32_t> idx({m, (py::ssize_t)k});
        const float *q = points.data();
        float *d = dist.mutable_data();
        uint32_t *i = idx.mutable_data();
        nbkd_status st;
        Interruptible intr;
        {
            py::gil_scoped_release nogil;
            st = nbkd_query_knn(h_, q, (uint64_t)m, k, d, i, 0u, nullptr);
        }
        intr.finish(st);
        return {dist, idx};
    }

    // distance to the k-th neighbour only (nbkd_query_kth), float32 (m,)
    py::array_t<float> query_kth(farray points, int k) {
        if (k <= 0) throw std::runtime_error("k must be positive integer");
        check_shape(points);
        const py::ssize_t m = points.shape(0);
        py::array_t<float> out(m);
        const float *q = points.data();
        float *o = out.mutable_data();
        nbkd_status st;
        Interruptible intr;
        {
            py::gil_scoped_release nogil;
            st = nbkd_query_kth(h_, q, (uint64_t)m, k, o, 0u, nullptr);
        }
        intr.finish(st);
        return out;
    }

    py::array_t<uint32_t> query_ball_count(farray points, float r) {
        check_shape(points);
        const py::ssize_t m = points.shape(0);
        py::array_t<uint32_t> out(m);
        const float *q = points.data();
        uint32_t *o = out.mutable_data();
        nbkd_status st;
        Interruptible intr;
        {
            py::gil_scoped_release nogil;
            st = nbkd_query_ball_count(h_, q, (uint64_t)m, r, o, 0u, nullptr);
        }
        intr.finish(st);
        return out;
    }

    // the radius count for nr ascending radii in one walk (nbkd_query_ball_hist):
    // (total uint64 (nr,), cumulative counts uint32 (m, nr) or None)
    py::tuple query_ball_hist(farray points, farray radii, bool per_point) {
        check_shape(points);
        if (radii.ndim() != 1) throw std::runtime_error("radii must be a 1D array");
        const py::ssize_t m = points.shape(0), nr = radii.shape(0);
        if (nr < 1 || nr > NBKD_MAX_RADII)
            throw std::runtime_error("the number of radii must be in [1, " +
                                     std::to_string(NBKD_MAX_RADII) + "]");
        py::array_t<uint64_t> total(nr);
        py::object counts = py::none();
        uint32_t *c = nullptr;
        if (per_point) {
            py::array_t<uint32_t> arr({m, nr});
            c = arr.mutable_data();
            counts = arr;
        }
        const float *q = points.data(), *r = radii.data();
        uint64_t *tp = total.mutable_data();
        // (m == 0: no array to point at; the library only zeroes the totals)
        const float dummy[3] = {0.0f, 0.0f, 0.0f};
        if (m == 0) q = dummy;
        nbkd_status st;
        Interruptible intr;
        {
            py::gil_scoped_release nogil;
            st = nbkd_query_ball_hist(h_, q, (uint64_t)m, r, (int32_t)nr, c, tp, 0u, nullptr);
        }
        intr.finish(st);
        return py::make_tuple(total, counts);
    }

    // anisotropic pair counts in one walk (nbkd_query_ball_hist2): the (n1, n2)
    // uint64 bins, (rp, pi) for mode 0 and (s, mu) for mode 1
    py::array_t<uint64_t> query_ball_hist2(farray points, farray edges1, farray edges2, int mode,
                                           int los) {
        check_shape(points);
        if (edges1.ndim() != 1 || edges2.ndim() != 1)
            throw std::runtime_error("the edges must be 1D arrays");
        const py::ssize_t m = points.shape(0), n1 = edges1.shape(0), n2 = edges2.shape(0);
        if (n1 < 1 || n1 > NBKD_MAX_RADII)
            throw std::runtime_error("the number of first-axis edges must be in [1, " +
                                     std::to_string(NBKD_MAX_RADII) + "]");
        if (n2 < 1 || n2 > NBKD_MAX_LOS_BINS)
            throw std::runtime_error("the number of second-axis edges must be in [1, " +
                                     std::to_string(NBKD_MAX_LOS_BINS) + "]");
        py::array_t<uint64_t> total({n1, n2});
        const float *q = points.data(), *e1 = edges1.data(), *e2 = edges2.data();
        uint64_t *tp = total.mutable_data();
        // (m == 0: no array to point at; the library only zeroes the totals)
        const float dummy[3] = {0.0f, 0.0f, 0.0f};
        if (m == 0) q = dummy;
        nbkd_status st;
        Interruptible intr;
        {
            py::gil_scoped_release nogil;
            st = nbkd_query_ball_hist2(h_, q, (uint64_t)m, (int32_t)mode, (int32_t)los, e1,
                                       (int32_t)n1, e2, (int32_t)n2, tp, 0u, nullptr);
        }
        intr.finish(st);
        return total;
    }

    // the same in the observer frame (nbkd_query_ball_hist2_obs): each pair's
    // line of sight from observer (3 floats) through the pair's midpoint
    py::array_t<uint64_t> query_ball_hist2_obs(farray points, farray edges1, farray edges2,
                                               int mode, farray observer) {
        check_shape(points);
        if (edges1.ndim() != 1 || edges2.ndim() != 1)
            throw std::runtime_error("the edges must be 1D arrays");
        if (observer.ndim() != 1 || observer.shape(0) != 3)
            throw std::runtime_error("observer must be a 1D array of 3 coordinates");
        const py::ssize_t m = points.shape(0), n1 = edges1.shape(0), n2 = edges2.shape(0);
        if (n1 < 1 || n1 > NBKD_MAX_RADII)
            throw std::runtime_error("the number of first-axis edges must be in [1, " +
                                     std::to_string(NBKD_MAX_RADII) + "]");
        if (n2 < 1 || n2 > NBKD_MAX_LOS_BINS)
            throw std::runtime_error("the number of second-axis edges must be in [1, " +
                                     std::to_string(NBKD_MAX_LOS_BINS) + "]");
        py::array_t<uint64_t> total({n1, n2});
        const float *q = points.data(), *e1 = edges1.data(), *e2 = edges2.data();
        const float *o = observer.data();
        uint64_t *tp = total.mutable_data();
        // (m == 0: no array to point at; the library only zeroes the totals)
        const float dummy[3] = {0.0f, 0.0f, 0.0f};
        if (m == 0) q = dummy;
        nbkd_status st;
        Interruptible intr;
        {
            py::gil_scoped_release nogil;
            st = nbkd_query_ball_hist2_obs(h_, q, (uint64_t)m, (int32_t)mode, o, e1, (int32_t)n1,
                                           e2, (int32_t)n2, tp, 0u, nullptr);
        }
        intr.finish(st);
        return total;
    }

    // kernel-weighted sums over each query's own ball (nbkd_query_ball_sum):
    // (raw float32 sums (m, nv), counts uint32 (m,) or None).  values: None
    // (weight 1, nv = 1) or an (N, nv) array by input row.
    py::tuple ball_sum(farray points, farray h, std::optional<farray> values, int kernel,
                       bool count) {
        check_shape(points);
        const py::ssize_t m = points.shape(0);
        if (h.ndim() != 1 || h.shape(0) != m)
            throw std::runtime_error("h must be a 1D array with one radius per query");
        py::ssize_t nv = 1;
        const float *v = nullptr;
        if (values.has_value()) {
            if (values->ndim() != 2 || (uint64_t)values->shape(0) != n_in_)
                throw std::runtime_error("values must be a 2D array of shape (N, nv)");
            nv = values->shape(1);
            v = values->data();
        }
        if (nv < 1 || nv > NBKD_MAX_VALUES)
            throw std::runtime_error("the number of value channels must be in [1, " +
                                     std::to_string(NBKD_MAX_VALUES) + "]");
        py::array_t<float> sums({m, nv});
        py::object counts = py::none();
        uint32_t *c = nullptr;
        if (count) {
            py::array_t<uint32_t> arr(m);
            c = arr.mutable_data();
            counts = arr;
        }
        const float *q = points.data(), *hp = h.data();
        float *sp = sums.mutable_data();
        // (m == 0: no arrays to point at; the library returns at once)
        const float dummy[3] = {0.0f, 0.0f, 0.0f};
        if (m == 0) q = hp = dummy;
        nbkd_status st;
        Interruptible intr;
        {
            py::gil_scoped_release nogil;
            st = nbkd_query_ball_sum(h_, q, (uint64_t)m, hp, v, (int32_t)nv, (int32_t)kernel, sp,
                                     c, 0u, nullptr);
        }
        intr.finish(st);
        return py::make_tuple(sums, counts);
    }

    // weighted radial profiles (nbkd_query_ball_profile): raw float32 per-bin
    // sums (m, nr, nv).  values: None (weight 1, nv = 1) or an (N, nv) array by
    // input row; scale: None or one factor per query.
    py::array_t<float> ball_profile(farray points, farray radii, std::optional<farray> values,
                                    std::optional<farray> scale) {
        check_shape(points);
        if (radii.ndim() != 1) throw std::runtime_error("radii must be a 1D array");
        const py::ssize_t m = points.shape(0), nr = radii.shape(0);
        if (nr < 1 || nr > NBKD_MAX_RADII)
            throw std::runtime_error("the number of radii must be in [1, " +
                                     std::to_string(NBKD_MAX_RADII) + "]");
        const float *sc = nullptr;
        if (scale.has_value()) {
            if (scale->ndim() != 1 || scale->shape(0) != m)
                throw std::runtime_error("scale must be a 1D array with one factor per query");
            sc = scale->data();
        }
        py::ssize_t nv = 1;
        const float *v = nullptr;
        if (values.has_value()) {
            if (values->ndim() != 2 || (uint64_t)values->shape(0) != n_in_)
                throw std::runtime_error("values must be a 2D array of shape (N, nv)");
            nv = values->shape(1);
            v = values->data();
        }
        if (nv < 1 || nv > NBKD_MAX_VALUES)
            throw std::runtime_error("the number of value channels must be in [1, " +
                                     std::to_string(NBKD_MAX_VALUES) + "]");
        py::array_t<float> sums({m, nr, nv});
        const float *q = points.data(), *r = radii.data();
        float *sp = sums.mutable_data();
        // (m == 0: no arrays to point at; the library returns at once)
        const float dummy[3] = {0.0f, 0.0f, 0.0f};
        float dummy_out[1];
        if (m == 0) {
            q = dummy;
            sp = dummy_out;
        }
        nbkd_status st;
        Interruptible intr;
        {
            py::gil_scoped_release nogil;
            st = nbkd_query_ball_profile(h_, q, (uint64_t)m, sc, r, (int32_t)nr, v, (int32_t)nv,
                                         sp, 0u, nullptr);
        }
        intr.finish(st);
        return sums;
    }

    // Barnes-Hut potentials and accelerations at the query points, G = 1
    // (nbkd_gravity): (phi float32 (m,) or None, acc float32 (m, 3) or None).
    // mass: None (mass 1) or an (N,) array by input row.
    py::tuple gravity(farray points, std::optional<farray> mass, float theta, float eps,
                      bool potential, bool acceleration) {
        return gravity_call(false, points, mass, theta, eps, potential, acceleration);
    }

    // the same on a periodic tree, with the Ewald correction (nbkd_gravity_ewald);
    // a query outside [0, L]^3 gets NaNs
    py::tuple gravity_ewald(farray points, std::optional<farray> mass, float theta, float eps,
                            bool potential, bool acceleration) {
        return gravity_call(true, points, mass, theta, eps, potential, acceleration);
    }

    py::tuple gravity_call(bool ewald, farray points, std::optional<farray> mass, float theta,
                           float eps, bool potential, bool acceleration) {
        check_shape(points);
        const py::ssize_t m = points.shape(0);
        const float *w = nullptr;
        if (mass.has_value()) {
            if (mass->ndim() != 1 || (uint64_t)mass->shape(0) != n_in_)
                throw std::runtime_error("mass must be a 1D array with one mass per point");
            w = mass->data();
        }
        if (!potential && !acceleration)
            throw std::runtime_error("at least one of potential and acceleration is needed");
        py::object phi = py::none(), acc = py::none();
        float *pp = nullptr, *ap = nullptr;
        if (potential) {
            py::array_t<float> arr(m);
            pp = arr.mutable_data();
            phi = arr;
        }
        if (acceleration) {
            py::array_t<float> arr({m, (py::ssize_t)3});
            ap = arr.mutable_data();
            acc = arr;
        }
        const float *q = points.data();
        // (m == 0: no array to point at; the library returns at once)
        const float dummy[3] = {0.0f, 0.0f, 0.0f};
        if (m == 0) q = dummy;
        nbkd_status st;
        Interruptible intr;
        {
            py::gil_scoped_release nogil;
            st = ewald ? nbkd_gravity_ewald(h_, q, (uint64_t)m, w, theta, eps, pp, ap, 0u, nullptr)
                       : nbkd_gravity(h_, q, (uint64_t)m, w, theta, eps, pp, ap, 0u, nullptr);
        }
        intr.finish(st);
        return py::make_tuple(phi, acc);
    }

    // friends-of-friends groups of the tree's points (nbkd_fof): (labels uint32
    // (N,) = the smallest input row of each point's group, sizes uint32 (N,) =
    // the member count at each label, 0 elsewhere)
    std::pair<py::array_t<uint32_t>, py::array_t<uint32_t>> fof_labels(float b) {
        py::array_t<uint32_t> labels((py::ssize_t)n_in_), sizes((py::ssize_t)n_in_);
        uint32_t *l = labels.mutable_data(), *z = sizes.mutable_data();
        nbkd_status st;
        {
            py::gil_scoped_release nogil;
            st = nbkd_fof(h_, b, l, z, nullptr, 0u, nullptr);
        }
        check(st);
        return {labels, sizes};
    }

    // the group catalogue of a canonical labelling (nbkd_group_catalog), sized
    // with one call and filled with a second: (head uint32 (G,), size uint32
    // (G,), offsets uint64 (G + 1,) or None, members uint32 (K,) or None,
    // moments float64 (G, 5 + 2 nv), dmax float32 (G,))
    py::tuple group_moments(py::array_t<uint32_t, py::array::c_style | py::array::forcecast> labels,
                            uint32_t min_members, std::optional<farray> weight,
                            std::optional<farray> values, bool members) {
        if (labels.ndim() != 1 || (uint64_t)labels.shape(0) != n_in_)
            throw std::runtime_error("labels must be a 1D array with one label per point");
        const float *w = nullptr, *v = nullptr;
        py::ssize_t nv = 0;
        if (weight.has_value()) {
            if (weight->ndim() != 1 || (uint64_t)weight->shape(0) != n_in_)
                throw std::runtime_error("weight must be a 1D array with one weight per point");
            w = weight->data();
        }
        if (values.has_value()) {
            if (values->ndim() != 2 || (uint64_t)values->shape(0) != n_in_)
                throw std::runtime_error("values must be a 2D array of shape (N, nv)");
            nv = values->shape(1);
            if (nv < 1 || nv > NBKD_MAX_VALUES)
                throw std::runtime_error("the number of value channels must be in [1, " +
                                         std::to_string(NBKD_MAX_VALUES) + "]");
            v = values->data();
        }
        const uint32_t *l = labels.data();
        uint64_t G = 0, K = 0;
        nbkd_status st;
        {
            py::gil_scoped_release nogil;
            st = nbkd_group_catalog(h_, l, w, v, (int32_t)nv, min_members, 0, 0, &G, &K, nullptr,
                                    nullptr, nullptr, nullptr, nullptr, nullptr, 0u, nullptr);
        }
        check(st);
        py::array_t<uint32_t> head((py::ssize_t)G), size((py::ssize_t)G);
        py::array_t<double> mom({(py::ssize_t)G, (py::ssize_t)NBKD_GROUP_MOMENTS(nv)});
        py::array_t<float> dmax((py::ssize_t)G);
        py::object offsets = py::none(), mem = py::none();
        uint64_t *op = nullptr;
        uint32_t *mp = nullptr;
        if (members) {
            py::array_t<uint64_t> o((py::ssize_t)G + 1);
            py::array_t<uint32_t> m((py::ssize_t)K);
            op = o.mutable_data();
            mp = m.mutable_data();
            op[0] = 0; // (G == 0: the library writes nothing)
            offsets = o;
            mem = m;
        }
        if (G > 0) {
            uint32_t *hp = head.mutable_data(), *sp = size.mutable_data();
            double *dp = mom.mutable_data();
            float *xp = dmax.mutable_data();
            uint64_t G2 = 0, K2 = 0;
            {
                py::gil_scoped_release nogil;
                st = nbkd_group_catalog(h_, l, w, v, (int32_t)nv, min_members, G, K, &G2, &K2, hp,
                                        sp, op, mp, dp, xp, 0u, nullptr);
            }
            check(st);
        }
        return py::make_tuple(head, size, offsets, mem, mom, dmax);
    }

    // per-entry potentials of a list of row groups and each group's entry of
    // lowest potential (nbkd_group_potential): (phi float32 (K,), minpos uint32
    // (G,), 0xFFFFFFFF for an empty or a skipped group)
    py::tuple group_potential(
        py::array_t<uint64_t, py::array::c_style | py::array::forcecast> offsets,
        py::array_t<uint32_t, py::array::c_style | py::array::forcecast> members,
        std::optional<farray> mass, float eps, uint32_t max_members) {
        if (offsets.ndim() != 1 || offsets.shape(0) < 1)
            throw std::runtime_error("offsets must be a 1D array of ngroups + 1 entries");
        if (members.ndim() != 1) throw std::runtime_error("members must be a 1D array");
        const float *w = nullptr;
        if (mass.has_value()) {
            if (mass->ndim() != 1 || (uint64_t)mass->shape(0) != n_in_)
                throw std::runtime_error("mass must be a 1D array with one mass per point");
            w = mass->data();
        }
        const py::ssize_t G = offsets.shape(0) - 1, K = members.shape(0);
        py::array_t<float> phi(K);
        py::array_t<uint32_t> minpos(G);
        const uint64_t *op = offsets.data();
        // (K == 0: no array to point at; the library reads no member)
        const uint32_t dummy = 0;
        const uint32_t *mp = K ? members.data() : &dummy;
        float *pp = phi.mutable_data();
        uint32_t *ip = minpos.mutable_data();
        nbkd_status st;
        {
            py::gil_scoped_release nogil;
            st = nbkd_group_potential(h_, op, mp, (uint64_t)G, (uint64_t)K, w, eps, max_members,
                                      pp, ip, 0u, nullptr);
        }
        check(st);
        return py::make_tuple(phi, minpos);
    }

    // rows sorted ascending on the device unless sorted=false (NBKD_SORTED);
    // both passes stream in batches and poll Ctrl-C between them
    std::pair<py::array_t<uint64_t>, py::array_t<uint32_t>> query_ball_csr(farray points, float r,
                                                                           bool sorted) {
        check_shape(points);
        const py::ssize_t m = points.shape(0);
        py::array_t<uint64_t> off(m + 1);
        const float *q = points.data();
        uint64_t *o = off.mutable_data();
        const uint32_t fl = sorted ? NBKD_SORTED : 0u;
        nbkd_status st;
        {
            Interruptible intr;
            {
                py::gil_scoped_release nogil;
                st = nbkd_query_ball_csr(h_, q, (uint64_t)m, r, o, nullptr, 0, fl, nullptr);
            }
            intr.finish(st);
        }
        const uint64_t nnz = o[m];
        py::array_t<uint32_t> idx((py::ssize_t)nnz);
        uint32_t *ip = idx.mutable_data();
        {
            Interruptible intr;
            {
                py::gil_scoped_release nogil;
                st = nbkd_query_ball_csr(h_, q, (uint64_t)m, r, o, ip, nnz, fl, nullptr);
            }
            intr.finish(st);
        }
        return {off, idx};
    }

    // node table (n, 4) as raw 32-bit words + tree-ordered SoA, for parity tests
    py::tuple export_tree() const {
        py::array_t<uint32_t> nodes({(py::ssize_t)nodes_, (py::ssize_t)4});
        py::array_t<float> x((py::ssize_t)n8_), y((py::ssize_t)n8_), z((py::ssize_t)n8_);
        py::array_t<uint32_t> idx((py::ssize_t)n8_);
        check(nbkd_export(h_, reinterpret_cast<nbkd_node *>(nodes.mutable_data()),
                          x.mutable_data(), y.mutable_data(), z.mutable_data(),
                          idx.mutable_data()));
        return py::make_tuple(nodes, x, y, z, idx);
    }
};

} // namespace

PYBIND11_MODULE(_impl, m) {
    m.doc() = "MI355X-native KD-tree for spatial data, including periodic boundary conditions.";

    py::class_<PyKDTree>(m, "KDTree")
        .def(py::init<farray, int, int, std::optional<float>, int>(), py::arg("points"),
             py::arg("leafsize") = 64, py::arg("max_threads") = -1,
             py::arg("boxsize") = std::nullopt, py::arg("device") = -1)
        .def("query", &PyKDTree::query, py::arg("points"), py::arg("k") = 1,
             py::arg("workers") = 1)
        .def("query_kth", &PyKDTree::query_kth, py::arg("points"), py::arg("k"))
        .def("query_ball_count", &PyKDTree::query_ball_count, py::arg("points"), py::arg("r"))
        .def("query_ball_hist", &PyKDTree::query_ball_hist, py::arg("points"), py::arg("radii"),
             py::arg("per_point") = false)
        .def("query_ball_hist2", &PyKDTree::query_ball_hist2, py::arg("points"),
             py::arg("edges1"), py::arg("edges2"), py::arg("mode"), py::arg("los") = 2)
        .def("query_ball_hist2_obs", &PyKDTree::query_ball_hist2_obs, py::arg("points"),
             py::arg("edges1"), py::arg("edges2"), py::arg("mode"), py::arg("observer"))
        .def("query_ball_csr", &PyKDTree::query_ball_csr, py::arg("points"), py::arg("r"),
             py::arg("sorted") = true)
        .def("ball_sum", &PyKDTree::ball_sum, py::arg("points"), py::arg("h"),
             py::arg("values") = std::nullopt, py::arg("kernel") = NBKD_KERNEL_CUBIC,
             py::arg("count") = false)
        .def("ball_profile", &PyKDTree::ball_profile, py::arg("points"), py::arg("radii"),
             py::arg("values") = std::nullopt, py::arg("scale") = std::nullopt)
        .def("gravity", &PyKDTree::gravity, py::arg("points"), py::arg("mass") = std::nullopt,
             py::arg("theta") = 0.5f, py::arg("eps") = 0.0f, py::arg("potential") = true,
             py::arg("acceleration") = true)
        .def("gravity_ewald", &PyKDTree::gravity_ewald, py::arg("points"),
             py::arg("mass") = std::nullopt, py::arg("theta") = 0.5f, py::arg("eps") = 0.0f,
             py::arg("potential") = true, py::arg("acceleration") = true)
        .def("fof_labels", &PyKDTree::fof_labels, py::arg("b"))
        .def("group_moments", &PyKDTree::group_moments, py::arg("labels"),
             py::arg("min_members") = 1, py::arg("weight") = std::nullopt,
             py::arg("values") = std::nullopt, py::arg("members") = true)
        .def("group_potential", &PyKDTree::group_potential, py::arg("offsets"),
             py::arg("members"), py::arg("mass") = std::nullopt, py::arg("eps") = 0.0f,
             py::arg("max_members") = 0)
        .def("export", &PyKDTree::export_tree)
        .def_property_readonly("n", &PyKDTree::num_points)
        .def_property_readonly("size", &PyKDTree::num_nodes)
        .def_property_readonly("periodic", &PyKDTree::periodic)
        .def_property_readonly("boxsize", &PyKDTree::box_size)
        .def_property_readonly("device", &PyKDTree::device);

    m.def("device_count", []() {
        int32_t c = 0;
        nbkd_device_count(&c);
        return c;
    });
}
