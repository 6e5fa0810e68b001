// lane_park.h -- per-lane state of a stage body kept outside the registers across a stretch of the body that needs them.
//
// On the GPU: N doubles per lane in LDS columns of the layout of the traversal stacks (hip/exec.h: RDR_STACK_DECL), entry k of
// lane t at [k * 256 + t]: conflict-free.  A value parked and fetched back costs two LDS instructions per lane; the same value
// spilled by a register cap goes through scratch, i.e. HBM.  Declared once per stage body (RDR_PARK_DECL), after the point where
// inactive lanes have returned; a lane touches its own column only, so no barrier is needed.  256 x N x 8 bytes of LDS per
// workgroup: count them against the workgroups per CU the stage is compiled for (160 KiB per CU).
// On the host (the single-threaded debugging harness, tests/hostsim): a local array with the same interface, so that the harness
// runs the same stage source.
// V3 / V2 of vecmath.h go through put3 / get3<V3> / add3 and put2 / get2<V2> / add2: any struct of x, y(, z) doubles.
#pragma once

namespace rdr {
#if defined(__HIP__)
#define RDR_PARK_DECL(name, N) __shared__ double name##_lds[(N) * 256]; rdr::LanePark<N> name(name##_lds)
#define RDR_PARK_FN __host__ __device__
template <int N> struct LanePark {
    double *col;
    RDR_PARK_FN explicit LanePark(double *tile) : col(tile + threadIdx.x) {}
    // Reads go through a copy of the column pointer whose origin the optimiser cannot see: it must not forward the parked value
    // from the put to the get (that keeps it in a register for the whole stretch: the thing this is here to avoid).
    RDR_PARK_FN double *rd() const {
        double *p = col;
#if defined(__HIP_DEVICE_COMPILE__)
        asm("" : "+v"(p));
#endif
        return p;
    }
    RDR_PARK_FN void put(int k, double v) const { col[k * 256] = v; }
    RDR_PARK_FN double get(int k) const { return rd()[k * 256]; }
    RDR_PARK_FN void add(int k, double v) const { double *p = rd(); p[k * 256] = p[k * 256] + v; }
#else
#define RDR_PARK_DECL(name, N) rdr::LanePark<N> name
#define RDR_PARK_FN
template <int N> struct LanePark {
    mutable double slot[N];
    void put(int k, double v) const { slot[k] = v; }
    double get(int k) const { return slot[k]; }
    void add(int k, double v) const { slot[k] = slot[k] + v; }
#endif
    // the typed forms, the same on both sides
    template <int M> RDR_PARK_FN void put(int k, const double (&v)[M]) const {
        static_assert(M <= N, "more doubles than the park has columns");
        for (int i = 0; i < M; ++i) put(k + i, v[i]);
    }
    template <int M> RDR_PARK_FN void get(int k, double (&v)[M]) const { for (int i = 0; i < M; ++i) v[i] = get(k + i); }
    template <class V> RDR_PARK_FN void put3(int k, const V &v) const { put(k, v.x); put(k + 1, v.y); put(k + 2, v.z); }
    template <class V> RDR_PARK_FN V get3(int k) const { return V{get(k), get(k + 1), get(k + 2)}; }
    template <class V> RDR_PARK_FN V get3(int k, const V &) const { return get3<V>(k); }      // (the type from an argument)
    template <class V> RDR_PARK_FN void add3(int k, const V &v) const { add(k, v.x); add(k + 1, v.y); add(k + 2, v.z); }
    template <class V> RDR_PARK_FN void put2(int k, const V &v) const { put(k, v.x); put(k + 1, v.y); }
    template <class V> RDR_PARK_FN V get2(int k) const { return V{get(k), get(k + 1)}; }
    template <class V> RDR_PARK_FN void add2(int k, const V &v) const { add(k, v.x); add(k + 1, v.y); }
};
#undef RDR_PARK_FN
}
