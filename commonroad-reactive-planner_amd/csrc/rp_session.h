// rp_session.h -- the host session of the trajectory libraries, stated once: the first fields of an opaque object (device, stream,
// last error, the four blocks of a call), fail and RP_TRY, the growing block, align8, the upload of a table and what stands behind a
// library's create, destroy and last_error.  Host code only; it names no library: each one passes the prefix of its messages.
// Everything here has internal linkage, nothing of it is exported.
//
// What every library built on it promises: a set call that fails, refused or at hipMalloc / hipMemcpy, leaves the earlier tables in
// force -- the new table is built beside the old one, and the old one is freed only once the new one is whole.
#ifndef RP_SESSION_H
#define RP_SESSION_H

#include <hip/hip_runtime.h>

#include <initializer_list>
#include <new>
#include <string>
#include <vector>

#include "../../include/rp_amd.h"

namespace {

// a table on the device, freed with the object that holds it
struct RpTable {
    double *p = nullptr;
    RpTable() = default;
    RpTable(const RpTable &) = delete;
    RpTable &operator=(const RpTable &) = delete;
    ~RpTable() {
        if (p) (void)hipFree(p);
    }
};

// a block that grows on demand, pinned host memory or device memory; freed with the object that holds it
struct RpBlock {
    const bool pinned;
    void *p = nullptr;
    size_t cap = 0;
    explicit RpBlock(bool pinned_) : pinned(pinned_) {}
    RpBlock(const RpBlock &) = delete;
    RpBlock &operator=(const RpBlock &) = delete;
    ~RpBlock() {
        if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
    }
};

// what every opaque object starts with: `struct rp_xyz : RpSession { its tables }`
struct RpSession {
    int device = 0;
    hipStream_t stream = nullptr;   // nullptr: create failed, the object has no device
    std::string err;
    // inputs of a call: pinned host block and its device copy; the results on the device and a pinned host block for the part of
    // them a call asks for
    RpBlock h_in{true}, d_in{false}, h_out{true}, d_out{false};
};

inline int fail(RpSession *s, int code, const std::string &msg) {
    s->err = msg;
    return code;
}

#define RP_TRY(s, expr)                                                                       \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(s, RP_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));       \
    } while (0)

inline size_t align8(size_t v) { return (v + 7) & ~(size_t)7; }

inline int grow(RpSession *s, const char *who, RpBlock &b, size_t need) {
    if (need <= b.cap) return RP_OK;
    if (b.p) { RP_TRY(s, b.pinned ? hipHostFree(b.p) : hipFree(b.p)); b.p = nullptr; }
    b.cap = 0;
    const size_t want = need < 65536 ? 65536 : need + need / 4;
    if ((b.pinned ? hipHostMalloc(&b.p, want, hipHostMallocDefault) : hipMalloc(&b.p, want)) != hipSuccess) {
        b.p = nullptr;
        return fail(s, RP_ENOMEM, std::string(who) + (b.pinned ? ": pinned host memory" : ": device memory"));
    }
    b.cap = want;
    return RP_OK;
}

// the four blocks of a call: in_bytes on the host and on the device, back_bytes on the host, dev_bytes on the device
inline int grow_call(RpSession *s, const char *who, size_t in_bytes, size_t back_bytes, size_t dev_bytes) {
    int rc;
    if ((rc = grow(s, who, s->h_in, in_bytes)) != RP_OK) return rc;
    if ((rc = grow(s, who, s->d_in, in_bytes)) != RP_OK) return rc;
    if ((rc = grow(s, who, s->h_out, back_bytes)) != RP_OK) return rc;
    return grow(s, who, s->d_out, dev_bytes);
}

// a device copy of src (nullptr for an empty one) in `fresh`; nothing the object holds is touched
inline int upload(RpSession *s, double *&fresh, const std::vector<double> &src) {
    fresh = nullptr;
    if (src.empty()) return RP_OK;
    RP_TRY(s, hipMalloc((void **)&fresh, src.size() * sizeof(double)));
    const hipError_t e = hipMemcpy(fresh, src.data(), src.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(fresh);
        fresh = nullptr;
        return fail(s, RP_EHIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
    }
    return RP_OK;
}

// Replaces up to four tables by device copies of their sources, all of them or none: the stream is drained, every new table is
// uploaded beside the old one, and the old ones are freed only when all new ones are whole.
struct RpTableSource {
    RpTable *table;
    const std::vector<double> *src;
};

inline int replace_tables(RpSession *s, std::initializer_list<RpTableSource> sets) {
    RP_TRY(s, hipSetDevice(s->device));
    RP_TRY(s, hipStreamSynchronize(s->stream));
    double *fresh[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t n = 0;
    for (const RpTableSource &t : sets) {
        const int rc = n < 4 ? upload(s, fresh[n], *t.src) : fail(s, RP_EINVAL, "replace_tables: more than four tables");
        if (rc != RP_OK) {
            while (n > 0)
                if (fresh[--n]) (void)hipFree(fresh[n]);
            return rc;
        }
        ++n;
    }
    n = 0;
    for (const RpTableSource &t : sets) {
        if (t.table->p) (void)hipFree(t.table->p);
        t.table->p = fresh[n++];
    }
    return RP_OK;
}

// ---- behind xyz_create, xyz_destroy and xyz_last_error ---------------------------------------------------------------------------
template <class T>
int session_create(T **out, int device) {
    if (!out) return RP_EINVAL;
    *out = nullptr;
    T *s = new (std::nothrow) T();
    if (!s) return RP_ENOMEM;
    *out = s;   // returned even on failure so that last_error works; the caller destroys it
    s->device = device;
    int ndev = 0;
    RP_TRY(s, hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(s, RP_EINVAL, "no such HIP device");
    RP_TRY(s, hipSetDevice(device));
    RP_TRY(s, hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    return RP_OK;
}

template <class T>
void session_destroy(T *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    const hipStream_t stream = s->stream;
    if (stream) (void)hipStreamSynchronize(stream);
    delete s;   // its tables and the four blocks
    if (stream) (void)hipStreamDestroy(stream);
}

template <class T>
const char *session_last_error(const T *s, const char *null_object) {
    return s ? s->err.c_str() : null_object;
}

}  // namespace

#endif  // RP_SESSION_H
