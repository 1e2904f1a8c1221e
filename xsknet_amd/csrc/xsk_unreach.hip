// xsk_unreach.hip — the port-unreachable responder: xsk_gpu_unreach_dev() and xsk_gpu_unreach_serve_dev()
// (include/xsk_gpu.h, "Port-unreachable responder").  UDP datagrams for an address of the neighbour
// table on a port nobody listens on are rewritten in place into ICMP / ICMPv6 port unreachable; the serve call is the
// second consumer in the chain: replies go onto the owning port's TX ring, everything else onto the `rest` ring, and a
// budget word limits the errors a call sends.  The decision, the lane pieces of the rewrite and the serve plan are
// xsk_unreach.h's (host and device); the table and its search are xsk_neigh.h's.
//
// Two kernels.  The decision is a lane per entry, a few dependent byte reads; the rewrite is the part with bytes to
// move -- up to 1232 quoted bytes forward by 48, and a checksum over all of them -- and belongs to a whole wave
// (ur_wave_rewrite, xsk_unreach_device.h):
//   unreach_kernel:       256-thread workgroups, a lane per frame decides; each wave then walks the ballot of its reply
//                         lanes and rewrites one reply after the other, all 64 lanes on each.
//   unreach_serve_kernel: one 1024-thread workgroup, lane j owns entry j -- decide; rank among the eligible entries and
//                         LIMITED behind the budget; rank per destination and the stopping lane as neigh_serve_kernel;
//                         the lanes below it store their entries and leave their rewrites as jobs in LDS, slot = rank
//                         among the eligible; behind a barrier wave w takes jobs w, w + 16, ...; a fence and a barrier;
//                         wave 0 publishes the index words, the budget, the result and the counters.
// No workspace, no second launch, no atomic that hands out a slot.  Index words and the budget are read through the
// vector path (load_word).
#include <errno.h>

#include "../../include/xsk_gpu.h"
#include "xsk_gpu_internal.h"
#include "xsk_hip_util.h"
#include "xsk_neigh_device.h"
#include "xsk_ring_dev.h"
#include "xsk_ring_pack.h"
#include "xsk_ring_ports_device.h"
#include "xsk_steer.h"
#include "xsk_unreach.h"
#include "xsk_unreach_device.h"

using namespace xskgpu;

static_assert(sizeof(xsk_gpu_unreach_stats) == 64 && sizeof(xsk_gpu_unreach_result) == 32, "the ABI's layouts");
static_assert(sizeof(xsk_gpu_desc) == 16, "one 16-B load and store per descriptor");
static_assert(kNgMaxPorts == kStMaxPorts, "the partition of xsk_steer.h serves the ports");

namespace {

constexpr uint32_t kUrFrames = kCpFrames;  // frames (and threads) per workgroup of unreach_kernel
constexpr uint32_t kUrWaves = kCpWaves;
// The serve call's workgroup and ring order are the neighbour serve call's (xsk_neigh_device.h: kNgServeThreads,
// kNgServeWaves, kNgRings); the ring consumed stands where that call has the stack ring.
constexpr uint32_t kUrSrc = kNgStack;

// The counters of one wave into s_red[wave]: seen, UNREACH4s, UNREACH6s, reply bytes, LIMITED entries.
__device__ __forceinline__ void wave_counters(bool seen, const UrVerdict& v, u64 (*s_red)[kUrStatsWords]) {
    const u64 ms = __ballot(seen), m4 = __ballot(seen && v.verdict == XSK_GPU_UNREACH_UNREACH4),
              m6 = __ballot(seen && v.verdict == XSK_GPU_UNREACH_UNREACH6),
              ml = __ballot(seen && v.verdict == XSK_GPU_UNREACH_LIMITED);
    const u64 bytes = cp_wave_sum(seen && ur_is_reply(v.verdict) ? (u64)v.reply_len : 0ull);
    if (cp_lane() == 0) {
        s_red[cp_wave()][0] = (u64)__popcll(ms);
        s_red[cp_wave()][1] = (u64)__popcll(m4);
        s_red[cp_wave()][2] = (u64)__popcll(m6);
        s_red[cp_wave()][3] = bytes;
        s_red[cp_wave()][4] = (u64)__popcll(ml);
    }
}
// Behind the barrier: thread w < 5 adds the workgroup's sum of word w, when it is not zero.
template <uint32_t NW>
__device__ __forceinline__ void add_counters(const u64 (*s_red)[kUrStatsWords], xsk_gpu_unreach_stats* ustats) {
    const uint32_t w = threadIdx.x;
    if (w >= kUrStatsWords || !ustats) return;
    u64 sum = 0;
    for (uint32_t k = 0; k < NW; ++k) sum += s_red[k][w];
    if (sum) atomicAdd(reinterpret_cast<u64*>(ustats) + w, sum);
}

// A value of the wave's lane `src` in every lane (src is wave-uniform).
__device__ __forceinline__ uint32_t from_lane(uint32_t x, uint32_t src) {
    return (uint32_t)__builtin_amdgcn_readlane((int)x, (int)src);
}

__global__ __launch_bounds__(kUrFrames) void unreach_kernel(uint8_t* umem, uint64_t umem_size, const xsk_gpu_desc* descs,
                                                            const uint32_t* d_n, uint32_t n_max, uint32_t opts,
                                                            const xsk_gpu_neigh_entry* table, uint32_t n_entries,
                                                            uint32_t n_ports, const uint64_t* d_bound,
                                                            const uint8_t* d_open, uint32_t chunk_size,
                                                            uint8_t* uverdicts, uint8_t* uports, uint32_t* reply_len,
                                                            xsk_gpu_unreach_stats* ustats) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_tab[];  // n_entries staged entries
    __shared__ u64 s_red[kUrWaves][kUrStatsWords];
    const uint32_t t = threadIdx.x;
    for (uint32_t k = t; k < n_entries; k += kUrFrames) ng_stage_entry(table + k, s_tab + k * kNgEntryWords);
    const u64 bound = d_bound ? *d_bound : ~0ull;
    const uint32_t n = d_n ? rd_min(*d_n, n_max) : n_max;
    __syncthreads();
    const uint32_t i = blockIdx.x * kUrFrames + t;  // below 2^32: n_max <= XSK_GPU_MAX_BATCH
    const bool seen = i < n;
    UrVerdict v = ur_none();
    uint64_t addr = 0;
    if (seen) {
        const xsk_gpu_desc d = ng_desc_of(reinterpret_cast<const uint4*>(descs)[i]);
        addr = d.addr;
        v = ur_decide(umem, umem_size, d, opts, s_tab, n_entries, n_ports, bound, d_open, chunk_size);
        if (ur_is_reply(v.verdict) && reply_len) reply_len[i] = v.reply_len;
        uverdicts[i] = (uint8_t)v.verdict;
        uports[i] = (uint8_t)v.port;
    }
    // the wave's replies, one after the other, every lane on each (wave-uniform loop)
    for (u64 todo = __ballot(seen && ur_is_reply(v.verdict)); todo; todo &= todo - 1ull) {
        const uint32_t src = (uint32_t)__builtin_ctzll(todo);
        UrVerdict w = ur_none();
        w.verdict = from_lane(v.verdict, src);
        w.l3 = from_lane(v.l3, src);
        w.q = from_lane(v.q, src);
        w.mac_lo = from_lane(v.mac_lo, src);
        w.mac_hi = from_lane(v.mac_hi, src);
        const uint64_t a = ((uint64_t)from_lane((uint32_t)(addr >> 32), src) << 32) | from_lane((uint32_t)addr, src);
        ur_wave_rewrite(umem + a, w);
    }
    if (!ustats) return;  // (uniform)
    wave_counters(seen, v, s_red);
    __syncthreads();
    add_counters<kUrWaves>(s_red, ustats);
}

// The serve kernel's arguments, one struct by value: 66 packed rings are 1584 B.
struct ServeArgs {
    PackedRing ring[kNgRings];  // tx[0 .. 64) (ports at or above n_ports: the absent ring), rest, up
    uint8_t* umem;
    uint64_t umem_size;
    const xsk_gpu_neigh_entry* table;
    const uint64_t* d_bound;
    const uint8_t* d_open;
    uint32_t* d_budget;
    xsk_gpu_unreach_stats* d_ustats;
    xsk_gpu_unreach_result* d_res;
    uint32_t n_ports, max, opts, n_entries, chunk_size;
};
static_assert(sizeof(ServeArgs) <= 4096, "the kernel arguments");

__device__ __forceinline__ Ring ring_dev(const PackedRing& p) {
    const UnpackedRing u = pk_unpack(p);
    return Ring{(uint32_t*)u.prod, (uint32_t*)u.cons, (void*)u.ring, u.size};
}

__global__ __launch_bounds__(kNgServeThreads) void unreach_serve_kernel(ServeArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_tab[];
    __shared__ Ring s_ring[kNgRings];
    __shared__ uint32_t s_cnt[kNgServeWaves][kStMaxPorts];
    __shared__ u64 s_red[kNgServeWaves][kUrStatsWords];
    __shared__ UrJob s_job[kNgServeThreads];
    __shared__ uint32_t s_prod[kNgDests], s_room[kNgDests];
    __shared__ uint32_t s_we[kNgServeWaves], s_wu[kNgServeWaves], s_wstop[kNgServeWaves];
    __shared__ uint32_t s_cons, s_used, s_budget;
    const uint32_t t = threadIdx.x;
    for (uint32_t k = t; k < A.n_entries; k += kNgServeThreads) ng_stage_entry(A.table + k, s_tab + k * kNgEntryWords);
    (&s_cnt[0][0])[t] = 0u;
    if (t < kNgRings) {  // a lane per ring: unpack, and the index words as they are at execution
        const Ring r = ring_dev(A.ring[t]);
        s_ring[t] = r;
        if (t == kUrSrc) {
            const uint32_t cons = load_word(r.cons);
            s_cons = cons;
            s_used = rd_used(load_word(r.prod), cons, r.size);
        } else if (t == kNgUp || t < A.n_ports) {
            const uint32_t prod = load_word(r.prod);
            s_prod[t] = prod;
            s_room[t] = rd_free(prod, load_word(r.cons), r.size);
        } else {
            s_prod[t] = 0u;
            s_room[t] = 0u;
        }
    }
    if (t == kNgRings) s_budget = A.d_budget ? load_word(A.d_budget) : 0xFFFFFFFFu;  // (at most 1024 are spent)
    const u64 bound = A.d_bound ? *A.d_bound : ~0ull;
    __syncthreads();
    // 1. every lane decides its entry
    const uint32_t m = ng_serve_m(s_used, A.max);
    const bool live = t < m;
    UrVerdict v = ur_none();
    uint4 raw = make_uint4(0u, 0u, 0u, 0u);
    if (live) {
        raw = *desc_slot(s_ring[kUrSrc], s_cons + t);
        v = ur_decide(A.umem, A.umem_size, ng_desc_of(raw), A.opts, s_tab, A.n_entries, A.n_ports, bound, A.d_open,
                      A.chunk_size);
    }
    // 2. the rank among the eligible entries; behind the budget an entry is LIMITED
    const bool eligible = live && ur_is_reply(v.verdict);
    const u64 me = cp_wg_ballot(eligible, s_we);
    const uint32_t erank = cp_waves_below<kNgServeWaves>(s_we, cp_wave(), 0u) + cp_below(me, cp_lane());
    const uint32_t budget = s_budget;
    v.verdict = ur_limit(v.verdict, erank, budget);
    // 3. the rank among the lower entries with the same destination
    const bool reply = live && ur_is_reply(v.verdict);
    const uint32_t port = reply ? v.port & (kStMaxPorts - 1u) : 0u;  // (a reply's port is below n_ports <= 64)
    const uint32_t in_wave = wave_ranks(reply, port, s_cnt);
    const u64 mu = cp_wg_ballot(live && !reply, s_wu);
    const uint32_t dest = ur_dest(v.verdict, port);  // (a lane without an entry: NONE, rest; it is not below m)
    const uint32_t rank = reply ? st1_lower_waves(s_cnt, cp_wave(), port) + in_wave
                                : cp_waves_below<kNgServeWaves>(s_wu, cp_wave(), 0u) + cp_below(mu, cp_lane());
    // 4. c: the lowest lane whose rank is not below its destination's room
    const u64 ms = __ballot(ng_stop_at(t, m, rank, s_room[dest]) != m);
    if (cp_lane() == 0) s_wstop[cp_wave()] = ms ? cp_wave() * kStWave + (uint32_t)__builtin_ctzll(ms) : m;
    __syncthreads();
    uint32_t c = m;
    for (uint32_t k = 0; k < kNgServeWaves; ++k) c = rd_min(c, s_wstop[k]);
    // 5. the lanes below c store their entries; a reply leaves its rewrite as job `erank` (below c the replies are the
    //    eligible entries of rank 0 .. n-1: erank < budget, and every eligible entry in front of one is below c too)
    const bool handled = t < c;
    if (handled) {
        const xsk_gpu_desc e = ng_desc_of(raw);
        if (reply) s_job[erank] = ur_job(e.addr, v);
        const xsk_gpu_desc o = ur_out_entry(e, v);
        *desc_slot(s_ring[dest], s_prod[dest] + rank) =
            make_uint4((uint32_t)o.addr, (uint32_t)(o.addr >> 32), o.len, o.options);
    }
    // what every port received: the partition again over the handled replies (see neigh_serve_kernel)
    (&s_cnt[0][0])[t] = 0u;
    wave_ranks(reply && handled, port, s_cnt);
    wave_counters(handled, v, s_red);
    __syncthreads();
    // 6. the rewrites, a wave each, round-robin
    uint32_t n_jobs = 0;
    for (uint32_t k = 0; k < kNgServeWaves; ++k) n_jobs += (uint32_t)(s_red[k][1] + s_red[k][2]);
    for (uint32_t j = cp_wave(); j < n_jobs; j += kNgServeWaves) {  // (wave-uniform)
        const UrJob job = s_job[j];
        ur_wave_rewrite(A.umem + ur_job_addr(job), ur_job_verdict(job));
    }
    __threadfence();  // the entries and the frames before the words that cover them
    __syncthreads();
    // 7. wave 0 publishes
    if (t >= kStWave) return;
    if (t < A.n_ports) {
        const uint32_t got = st1_port_total(s_cnt, t);
        if (got) *s_ring[t].prod = s_prod[t] + got;
    }
    if (t == 0) {
        u64 u4 = 0, u6 = 0, lim = 0;
        for (uint32_t k = 0; k < kNgServeWaves; ++k) {
            u4 += s_red[k][1];
            u6 += s_red[k][2];
            lim += s_red[k][4];
        }
        const uint32_t n_rest = c - n_jobs;
        if (n_rest) *s_ring[kNgUp].prod = s_prod[kNgUp] + n_rest;
        if (c) *s_ring[kUrSrc].cons = s_cons + c;
        if (A.d_budget && n_jobs) *A.d_budget = budget - n_jobs;
        if (A.d_res) {
            A.d_res->consumed = c;
            A.d_res->unreach4 = (uint32_t)u4;
            A.d_res->unreach6 = (uint32_t)u6;
            A.d_res->rest = n_rest;
            A.d_res->backlog = s_used - c;
            A.d_res->limited = (uint32_t)lim;
            A.d_res->reserved[0] = 0u;
            A.d_res->reserved[1] = 0u;
        }
    }
    add_counters<kNgServeWaves>(s_red, A.d_ustats);
}

// The rules the two calls add to the neighbour responder's.
bool extra_ok(const uint8_t* d_open, uint32_t chunk_size, const xsk_gpu_unreach_stats* d_ustats) {
    return ur_chunk_ok(chunk_size) && !((uintptr_t)d_open & 3u) && !((uintptr_t)d_ustats & 7u);
}

bool list_ok(const void* d_umem, const xsk_gpu_desc* d_descs, const uint32_t* d_n, uint32_t n_max, uint32_t opts,
             const xsk_gpu_neigh_entry* d_table, uint32_t n_entries, uint32_t n_ports, const uint64_t* d_bound,
             const uint8_t* d_uverdicts, const uint8_t* d_uports, const uint32_t* d_reply_len) {
    if (!d_umem || (opts & ~XSK_GPU_OPT_MASK) || n_ports < 1u || n_ports > kNgMaxPorts) return false;
    if (n_entries > kNgMaxEntries || (n_entries && !d_table) || ((uintptr_t)d_table & 7u) || ((uintptr_t)d_bound & 7u))
        return false;
    if (!d_descs || ((uintptr_t)d_descs & 15u) || !d_uverdicts || !d_uports || n_max > XSK_GPU_MAX_BATCH) return false;
    return !((uintptr_t)d_n & 3u) && !((uintptr_t)d_reply_len & 3u);
}

PackedRing pack(const xsk_gpu_ring_dev* r) {
    return pk_pack((uint64_t)(uintptr_t)r->d_producer, (uint64_t)(uintptr_t)r->d_consumer, (uint64_t)(uintptr_t)r->d_ring,
                   r->size);
}

// The launches; every argument has been checked.
int unreach_launch(void* d_umem, uint64_t umem_size, const xsk_gpu_desc* d_descs, const uint32_t* d_n, uint32_t n_max,
                   uint32_t opts, const xsk_gpu_neigh_entry* d_table, uint32_t n_entries, uint32_t n_ports,
                   const uint64_t* d_bound, const uint8_t* d_open, uint32_t chunk_size, uint8_t* d_uverdicts,
                   uint8_t* d_uports, uint32_t* d_reply_len, xsk_gpu_unreach_stats* d_ustats, hipStream_t s) {
    if (n_max == 0) return 0;
    const size_t lds = (size_t)n_entries * kNgEntryWords * sizeof(uint32_t);
    unreach_kernel<<<dim3(cp_nwg(n_max)), dim3(kUrFrames), lds, s>>>((uint8_t*)d_umem, umem_size, d_descs, d_n, n_max, opts,
                                                                     d_table, n_entries, n_ports, d_bound, d_open,
                                                                     chunk_size, d_uverdicts, d_uports, d_reply_len,
                                                                     d_ustats);
    HIP_TRY(hipGetLastError());
    return 0;
}

int serve_launch(const ServeArgs& a, hipStream_t s) {
    const size_t lds = (size_t)a.n_entries * kNgEntryWords * sizeof(uint32_t);
    unreach_serve_kernel<<<dim3(1), dim3(kNgServeThreads), lds, s>>>(a);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int xsk_gpu_unreach_dev(void* d_umem, uint64_t umem_size, const struct xsk_gpu_desc* d_descs, const uint32_t* d_n,
                        uint32_t n_max, uint32_t opts, const struct xsk_gpu_neigh_entry* d_table, uint32_t n_entries,
                        uint32_t n_ports, const uint64_t* d_bound, const uint8_t* d_open, uint32_t chunk_size,
                        uint8_t* d_uverdicts, uint8_t* d_uports, uint32_t* d_reply_len,
                        struct xsk_gpu_unreach_stats* d_ustats, void* stream) {
    if (!list_ok(d_umem, d_descs, d_n, n_max, opts, d_table, n_entries, n_ports, d_bound, d_uverdicts, d_uports,
                 d_reply_len) ||
        !extra_ok(d_open, chunk_size, d_ustats))
        return -EINVAL;
    return unreach_launch(d_umem, umem_size, d_descs, d_n, n_max, opts, d_table, n_entries, n_ports, d_bound, d_open,
                          chunk_size, d_uverdicts, d_uports, d_reply_len, d_ustats, (hipStream_t)stream);
}

int xsk_gpu_unreach_serve_dev(void* d_umem, uint64_t umem_size, const struct xsk_gpu_ring_dev* up,
                              const struct xsk_gpu_ring_dev* tx, uint32_t n_ports, const struct xsk_gpu_ring_dev* rest,
                              uint32_t max, uint32_t opts, const struct xsk_gpu_neigh_entry* d_table, uint32_t n_entries,
                              const uint64_t* d_bound, const uint8_t* d_open, uint32_t chunk_size, uint32_t* d_budget,
                              struct xsk_gpu_unreach_stats* d_ustats, struct xsk_gpu_unreach_result* d_res, void* stream) {
    // the ring, table, option, port, max, d_bound and d_res rules are the neighbour serve call's, stated there
    if (!xsk_gpu__serve_ok(d_umem, up, tx, n_ports, rest, max, opts, d_table, n_entries, d_bound, NULL,
                           (const struct xsk_gpu_neigh_result*)d_res) ||
        !extra_ok(d_open, chunk_size, d_ustats) || ((uintptr_t)d_budget & 3u))
        return -EINVAL;
    ServeArgs a;
    for (uint32_t p = 0; p < kNgMaxPorts; ++p) a.ring[p] = p < n_ports ? pack(tx + p) : pk_pack(0u, 0u, 0u, 1u);
    a.ring[kNgUp] = pack(rest);
    a.ring[kUrSrc] = pack(up);
    a.umem = (uint8_t*)d_umem;
    a.umem_size = umem_size;
    a.table = d_table;
    a.d_bound = d_bound;
    a.d_open = d_open;
    a.d_budget = d_budget;
    a.d_ustats = d_ustats;
    a.d_res = d_res;
    a.n_ports = n_ports;
    a.max = max;
    a.opts = opts;
    a.n_entries = n_entries;
    a.chunk_size = chunk_size;
    return serve_launch(a, (hipStream_t)stream);
}

}  // extern "C"
