// fir_class_cache.cpp -- the device class tables: built on the host (fir_class_table.cpp), uploaded once, cached per
// device and shared by every stream with the same polyphase table, rate pair, geometry and drift; and periodic_bind,
// which keeps a handle's table current.  HIP runtime API, no kernels.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>

#include "common.h"
#include "fir_periodic.h"

namespace rsmp {

namespace {

struct ClassTableKey {
    int device;
    const void* table;
    uint32_t den, a, b, row_len, mfma;
    uint64_t drift_bits;
    bool operator<(const ClassTableKey& o) const {
        return std::tie(device, table, den, a, b, row_len, mfma, drift_bits) <
               std::tie(o.device, o.table, o.den, o.a, o.b, o.row_len, o.mfma, o.drift_bits);
    }
};
struct ClassTableCache {
    std::mutex mu;
    struct Entry { ClassTable ct; uint64_t used; };
    std::map<ClassTableKey, Entry> tables;
    uint64_t tick = 0;
    static constexpr size_t kMaxTables = 96;    // (a geometry's table is 0.1-0.4 MB)
};
ClassTableCache& class_cache() {
    static ClassTableCache* c = new ClassTableCache;
    return *c;
}
// Device allocations of tables nobody holds any more.  Kernels enqueued earlier may still read them, so they are freed in
// batches, behind a hipDeviceSynchronize (class_table_for, on its slow path: a table is being built anyway).
struct ClassTableGraveyard {
    std::mutex mu;
    std::vector<std::pair<int, void*>> dead;   // (device, allocation)
    static constexpr size_t kPurgeAt = 32;
};
ClassTableGraveyard& class_graveyard() {
    static ClassTableGraveyard* g = new ClassTableGraveyard;
    return *g;
}
void purge_class_graveyard(int device) {
    ClassTableGraveyard& gy = class_graveyard();
    std::vector<std::pair<int, void*>> mine;
    {
        std::lock_guard<std::mutex> lock(gy.mu);
        if (gy.dead.size() < ClassTableGraveyard::kPurgeAt) return;
        for (auto it = gy.dead.begin(); it != gy.dead.end();) {
            if (it->first == device) { mine.push_back(*it); it = gy.dead.erase(it); }
            else ++it;
        }
    }
    if (mine.empty()) return;
    (void)hipDeviceSynchronize();   // (the current device is `device`: the callers' DeviceGuard)
    for (auto& d : mine) (void)hipFree(d.second);
}

constexpr double kDriftQuantum = 2e-9;  // positions this close share a class table

}  // namespace

int class_table_for(int device, const std::vector<float>& table, const PeriodicGeometry& g, double drift,
                    ClassTable* out, const HostClassTable* prebuilt) {
    ClassTableCache& cache = class_cache();
    std::lock_guard<std::mutex> lock(cache.mu);
    uint64_t bits;
    std::memcpy(&bits, &drift, sizeof bits);
    const ClassTableKey key{device, table.data(), g.den, g.a, g.b, g.row_len,
                            g.mfma == 3 ? 8u + g.planes : (g.mfma ? 1u : 0u), bits};
    auto it = cache.tables.find(key);
    if (it == cache.tables.end()) {
        purge_class_graveyard(device);
        if (cache.tables.size() >= ClassTableCache::kMaxTables) {   // the least recently used one leaves (its holders keep it alive)
            auto lru = cache.tables.begin();
            for (auto e = cache.tables.begin(); e != cache.tables.end(); ++e)
                if (e->second.used < lru->second.used) lru = e;
            cache.tables.erase(lru);
        }
        const auto tb0 = std::chrono::steady_clock::now();
        HostClassTable built;
        if (!prebuilt) built = build_class_table(table, g, drift);   // (0.35-0.7 ms of host arithmetic; `prebuilt`: somebody did it ahead)
        const HostClassTable& host = prebuilt ? *prebuilt : built;
        const auto tb1 = std::chrono::steady_clock::now();
        const size_t coef_bytes = host.coef.size() * sizeof(float);
        const size_t wrap_bytes = host.wrap_coef.size() * sizeof(float);
        const size_t meta_bytes = host.meta.size() * sizeof(TileMeta);
        char* dptr = nullptr;
        RSMP_HIP_CHECK(hipMalloc(&dptr, coef_bytes + wrap_bytes + meta_bytes));
        RSMP_HIP_CHECK(hipMemcpy(dptr, host.coef.data(), coef_bytes, hipMemcpyHostToDevice));
        RSMP_HIP_CHECK(hipMemcpy(dptr + coef_bytes, host.wrap_coef.data(), wrap_bytes,
                                 hipMemcpyHostToDevice));
        RSMP_HIP_CHECK(hipMemcpy(dptr + coef_bytes + wrap_bytes, host.meta.data(), meta_bytes,
                                 hipMemcpyHostToDevice));
        ClassTable ct;
        ct.d_coef = reinterpret_cast<const float*>(dptr);
        ct.d_wrap_coef = reinterpret_cast<const float*>(dptr + coef_bytes);
        ct.d_meta = reinterpret_cast<const TileMeta*>(dptr + coef_bytes + wrap_bytes);
        ct.hold = std::shared_ptr<void>(dptr, [device](void* p) {
            ClassTableGraveyard& gy = class_graveyard();
            std::lock_guard<std::mutex> lock(gy.mu);
            gy.dead.emplace_back(device, p);
        });
        it = cache.tables.emplace(key, ClassTableCache::Entry{ct, 0}).first;
        static const bool verbose = rsmp::knob("RSMP_FIR_VERBOSE") != nullptr;
        if (verbose)
            fprintf(stderr, "[rsmp] class table a=%u b=%u drift %.3g: built in %.3f ms on the host, %zu KB allocated and uploaded in %.3f ms\n", g.a, g.b, drift,
                    std::chrono::duration<double, std::milli>(tb1 - tb0).count(), (coef_bytes + wrap_bytes + meta_bytes) >> 10,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb1).count());
    }
    it->second.used = ++cache.tick;
    *out = it->second.ct;
    return RSMP_OK;
}

int periodic_bind(PeriodicState& st, int device, const std::vector<float>& table, int kernel_mode,
                  const FirMirror& planned, double launch_drift, uint32_t channels, hipStream_t stream) {
    (void)stream;
    const bool allow_matrix = kernel_mode != RSMP_FIR_KERNEL_PERIODIC_VECTOR;
    if (!st.geo_valid || st.geo_mode != kernel_mode) {   // (rsmp_fir_set_kernel may switch between them)
        st.geo = periodic_geometry(planned.num(), planned.den(), static_cast<uint32_t>(planned.taps()),
                                   channels, allow_matrix, kernel_mode != RSMP_FIR_KERNEL_PERIODIC_F32);
        st.geo_valid = true;
        st.geo_mode = kernel_mode;
        st.table_valid = false;
    }
    if (!st.geo.ok) return fail(RSMP_ERR_INVALID_ARGUMENT, "periodic kernel: unsupported geometry");
    const double drift = std::round(launch_drift / kDriftQuantum) * kDriftQuantum;
    if (st.table_valid && drift == st.table_drift) return RSMP_OK;
    ClassTable ct;
    const int rc = class_table_for(device, table, st.geo, drift, &ct);
    if (rc != RSMP_OK) return rc;
    st.table = ct;
    st.table_valid = true;
    st.table_drift = drift;
    return RSMP_OK;
}

}  // namespace rsmp
