// xsk_neigh.hip — the neighbour responder: xsk_gpu_neigh_table_prepare(), xsk_gpu_neigh_dev() and
// xsk_gpu_neigh_serve_dev() (include/xsk_gpu.h, "Neighbour responder").  ARP requests and neighbour
// solicitations for the addresses of a sorted table of at most 1024 entries are rewritten into their replies in place;
// the serve call is the first consumer of the stack ring (xsk_gpu_rx_pass_step_dev()) that lives on the device: replies
// go onto the owning port's TX ring, everything else onto the `up` ring.  The decision, the lookup, the rewrites and
// the serve plan are xsk_neigh.h's (host and device).
//
// Two kernels, both latency bound (a few dependent byte reads per frame, at most 352 B summed), no MFMA:
//   neigh_kernel:       256-thread workgroups, a lane per frame; the table staged once per workgroup into LDS as eight
//                       dwords an entry (at most 32 KiB, dynamic: none with an empty table) and searched there; the
//                       counters reduced by wave ballots and one wave sum, threads 0-3 issue one atomic a word.
//   neigh_serve_kernel: one 1024-thread workgroup, lane j owns stack entry j -- decide; rank per destination (the
//                       one-workgroup partition of xsk_steer.h for the ports, one more ballot for `up`); the lowest
//                       lane whose rank is not below its destination's room is c; behind a barrier the lanes below c
//                       rewrite and store; a fence and a barrier; wave 0 publishes the index words.  The 66 rings travel
//                       packed in the kernel arguments (xsk_ring_pack.h).
// No workspace, no second launch, no wait between workgroups, no atomic that hands out a slot.  Index words are read
// through the vector path (load_word).
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/xsk_gpu.h"
#include "xsk_gpu_internal.h"
#include "xsk_hip_util.h"
#include "xsk_neigh.h"
#include "xsk_ring_dev.h"
#include "xsk_ring_pack.h"
#include "xsk_ring_ports_device.h"
#include "xsk_steer.h"

using namespace xskgpu;

static_assert(sizeof(xsk_gpu_neigh_entry) == 24 && sizeof(xsk_gpu_neigh_stats) == 32 && sizeof(xsk_gpu_neigh_result) == 32,
              "the ABI's layouts");
static_assert(sizeof(xsk_gpu_desc) == 16, "one 16-B load and store per descriptor");
static_assert(kNgMaxPorts == kStMaxPorts && kNgMaxPorts == kEpMaxPorts, "the partition of xsk_steer.h serves the ports");

namespace {

typedef unsigned long long u64;

constexpr uint32_t kNgFrames = kCpFrames;  // frames (and threads) per workgroup of neigh_kernel
constexpr uint32_t kNgWaves = kCpWaves;
constexpr uint32_t kNgServeThreads = kSt1Frames;  // the serve call's one workgroup
constexpr uint32_t kNgServeWaves = kSt1Waves;
constexpr uint32_t kNgStack = kNgDests;           // the stack ring's place behind the 65 destinations
constexpr uint32_t kNgRings = kNgDests + 1u;
static_assert(kNgServeThreads == XSK_GPU_LOWLAT_MAX && kNgServeWaves * kStMaxPorts == kNgServeThreads,
              "a lane per entry, and a lane per word of the count matrix");

// The counters of one wave into s_red[wave]: seen, ARP replies, NAs, reply bytes.
__device__ __forceinline__ void wave_counters(bool seen, const NgVerdict& v, u64 (*s_red)[4]) {
    const u64 ms = __ballot(seen), ma = __ballot(seen && v.verdict == XSK_GPU_NEIGH_ARP_REPLY),
              mn = __ballot(seen && v.verdict == XSK_GPU_NEIGH_NA_REPLY);
    const u64 bytes = cp_wave_sum(seen && ng_is_reply(v.verdict) ? (u64)v.reply_len : 0ull);
    if (cp_lane() == 0) {
        s_red[cp_wave()][0] = (u64)__popcll(ms);
        s_red[cp_wave()][1] = (u64)__popcll(ma);
        s_red[cp_wave()][2] = (u64)__popcll(mn);
        s_red[cp_wave()][3] = bytes;
    }
}
// Behind the barrier: thread w < 4 adds the workgroup's sum of word w, when it is not zero.
template <uint32_t NW>
__device__ __forceinline__ void add_counters(const u64 (*s_red)[4], xsk_gpu_neigh_stats* nstats) {
    const uint32_t w = threadIdx.x;
    if (w >= 4u || !nstats) return;
    u64 sum = 0;
    for (uint32_t k = 0; k < NW; ++k) sum += s_red[k][w];
    if (sum) atomicAdd(reinterpret_cast<u64*>(nstats) + w, sum);
}

__device__ __forceinline__ xsk_gpu_desc desc_of(const uint4& r) {
    xsk_gpu_desc d;
    d.addr = ((uint64_t)r.y << 32) | r.x;
    d.len = r.z;
    d.options = r.w;
    return d;
}

__global__ __launch_bounds__(kNgFrames) void neigh_kernel(uint8_t* umem, uint64_t umem_size, const xsk_gpu_desc* descs,
                                                          const uint32_t* d_n, uint32_t n_max, uint32_t opts,
                                                          const xsk_gpu_neigh_entry* table, uint32_t n_entries,
                                                          uint32_t n_ports, const uint64_t* d_bound, uint8_t* nverdicts,
                                                          uint8_t* nports, uint32_t* reply_len,
                                                          xsk_gpu_neigh_stats* nstats) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_tab[];  // n_entries staged entries
    __shared__ u64 s_red[kNgWaves][4];
    const uint32_t t = threadIdx.x;
    for (uint32_t k = t; k < n_entries; k += kNgFrames) ng_stage_entry(table + k, s_tab + k * kNgEntryWords);
    const u64 bound = d_bound ? *d_bound : ~0ull;
    const uint32_t n = d_n ? rd_min(*d_n, n_max) : n_max;
    __syncthreads();
    const uint32_t i = blockIdx.x * kNgFrames + t;  // below 2^32: n_max <= XSK_GPU_MAX_BATCH
    const bool seen = i < n;
    NgVerdict v = {XSK_GPU_NEIGH_NONE, 0xFFu, 0u, 14u, 0u, 0u};
    if (seen) {
        const xsk_gpu_desc d = desc_of(reinterpret_cast<const uint4*>(descs)[i]);
        v = ng_decide(umem, umem_size, d, opts, s_tab, n_entries, n_ports, bound);
        if (ng_is_reply(v.verdict)) {
            ng_rewrite(umem + d.addr, v);
            if (reply_len) reply_len[i] = v.reply_len;
        }
        nverdicts[i] = (uint8_t)v.verdict;
        nports[i] = (uint8_t)v.port;
    }
    if (!nstats) return;  // (uniform)
    wave_counters(seen, v, s_red);
    __syncthreads();
    add_counters<kNgWaves>(s_red, nstats);
}

// The serve kernel's arguments, one struct by value: 66 packed rings are 1584 B.
struct ServeArgs {
    PackedRing ring[kNgRings];  // tx[0 .. 64) (ports at or above n_ports: the absent ring), up, stack
    uint8_t* umem;
    uint64_t umem_size;
    const xsk_gpu_neigh_entry* table;
    const uint64_t* d_bound;
    xsk_gpu_neigh_stats* d_nstats;
    xsk_gpu_neigh_result* d_res;
    uint32_t n_ports, max, opts, n_entries;
};
static_assert(sizeof(ServeArgs) <= 4096, "the kernel arguments");

__device__ __forceinline__ Ring ring_dev(const PackedRing& p) {
    const UnpackedRing u = pk_unpack(p);
    return Ring{(uint32_t*)u.prod, (uint32_t*)u.cons, (void*)u.ring, u.size};
}

// The body below is also ng_serve_body(), xsk_neigh_device.h, which the responder kernels call (xsk_responder_body.h).
// Called from here, with the LDS objects handed in, the compiler emitted the same 2084 instructions in another order
// (operands of additions commuted, address computations scheduled ahead of the values stored there:
// profiles/responder/README.md), so this kernel keeps its own text, as egress_ports_small_kernel does, and
// tests/test_responder_spec.py holds the two texts against each other.
__global__ __launch_bounds__(kNgServeThreads) void neigh_serve_kernel(ServeArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_tab[];
    __shared__ Ring s_ring[kNgRings];
    __shared__ uint32_t s_cnt[kNgServeWaves][kStMaxPorts];
    __shared__ u64 s_red[kNgServeWaves][4];
    __shared__ uint32_t s_prod[kNgDests], s_room[kNgDests];
    __shared__ uint32_t s_wu[kNgServeWaves], s_wstop[kNgServeWaves];
    __shared__ uint32_t s_cons, s_used;
    const uint32_t t = threadIdx.x;
    for (uint32_t k = t; k < A.n_entries; k += kNgServeThreads) ng_stage_entry(A.table + k, s_tab + k * kNgEntryWords);
    (&s_cnt[0][0])[t] = 0u;
    if (t < kNgRings) {  // a lane per ring: unpack, and the index words as they are at execution
        const Ring r = ring_dev(A.ring[t]);
        s_ring[t] = r;
        if (t == kNgStack) {
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
    const u64 bound = A.d_bound ? *A.d_bound : ~0ull;
    __syncthreads();
    // 1. every lane decides its entry
    const uint32_t m = ng_serve_m(s_used, A.max);
    const bool live = t < m;
    NgVerdict v = {XSK_GPU_NEIGH_NONE, 0xFFu, 0u, 14u, 0u, 0u};
    uint4 raw = make_uint4(0u, 0u, 0u, 0u);
    if (live) {
        raw = *desc_slot(s_ring[kNgStack], s_cons + t);
        v = ng_decide(A.umem, A.umem_size, desc_of(raw), A.opts, s_tab, A.n_entries, A.n_ports, bound);
    }
    // 2. the rank among the lower entries with the same destination
    const bool reply = live && ng_is_reply(v.verdict);
    const uint32_t port = reply ? v.port & (kStMaxPorts - 1u) : 0u;  // (a reply's port is below n_ports <= 64)
    const uint32_t in_wave = wave_ranks(reply, port, s_cnt);
    const u64 mu = cp_wg_ballot(live && !reply, s_wu);
    const uint32_t dest = ng_dest(v.verdict, port);  // (a lane without an entry: NONE, up; it is not below m)
    const uint32_t rank = reply ? st1_lower_waves(s_cnt, cp_wave(), port) + in_wave
                                : cp_waves_below<kNgServeWaves>(s_wu, cp_wave(), 0u) + cp_below(mu, cp_lane());
    // 3. c: the lowest lane whose rank is not below its destination's room
    const u64 ms = __ballot(ng_stop_at(t, m, rank, s_room[dest]) != m);
    if (cp_lane() == 0) s_wstop[cp_wave()] = ms ? cp_wave() * kStWave + (uint32_t)__builtin_ctzll(ms) : m;
    __syncthreads();
    uint32_t c = m;
    for (uint32_t k = 0; k < kNgServeWaves; ++k) c = rd_min(c, s_wstop[k]);
    // 4. the lanes below c rewrite and store
    const bool handled = t < c;
    if (handled) {
        const xsk_gpu_desc e = desc_of(raw);
        if (reply) ng_rewrite(A.umem + e.addr, v);
        const xsk_gpu_desc o = ng_out_entry(e, v);
        *desc_slot(s_ring[dest], s_prod[dest] + rank) =
            make_uint4((uint32_t)o.addr, (uint32_t)(o.addr >> 32), o.len, o.options);
    }
    // what every port received: the partition again over the handled replies.  A thread zeroes a word of its own
    // wave's row, which only its own wave writes; every read of the first matrix lies in front of the barrier above.
    (&s_cnt[0][0])[t] = 0u;
    wave_ranks(reply && handled, port, s_cnt);
    wave_counters(handled, v, s_red);
    __threadfence();  // the entries before the words that cover them
    __syncthreads();
    // 5. wave 0 publishes
    if (t >= kStWave) return;
    if (t < A.n_ports) {
        const uint32_t got = st1_port_total(s_cnt, t);
        if (got) *s_ring[t].prod = s_prod[t] + got;
    }
    if (t == 0) {
        u64 arp = 0, na = 0;
        for (uint32_t k = 0; k < kNgServeWaves; ++k) {
            arp += s_red[k][1];
            na += s_red[k][2];
        }
        const uint32_t n_up = c - (uint32_t)arp - (uint32_t)na;
        if (n_up) *s_ring[kNgUp].prod = s_prod[kNgUp] + n_up;
        if (c) *s_ring[kNgStack].cons = s_cons + c;
        if (A.d_res) {
            A.d_res->consumed = c;
            A.d_res->arp_replies = (uint32_t)arp;
            A.d_res->na_replies = (uint32_t)na;
            A.d_res->up = n_up;
            A.d_res->backlog = s_used - c;
            A.d_res->reserved[0] = 0u;
            A.d_res->reserved[1] = 0u;
            A.d_res->reserved[2] = 0u;
        }
    }
    add_counters<kNgServeWaves>(s_red, A.d_nstats);
}

int entry_cmp(const void* a, const void* b) {
    const xsk_gpu_neigh_entry* x = (const xsk_gpu_neigh_entry*)a;
    const xsk_gpu_neigh_entry* y = (const xsk_gpu_neigh_entry*)b;
    if (x->family != y->family) return x->family < y->family ? -1 : 1;
    return memcmp(x->addr, y->addr, 16);
}

bool entry_ok(const xsk_gpu_neigh_entry* e) {
    if ((e->family != 4 && e->family != 6) || e->port >= kNgMaxPorts || (e->mac[0] & 1u)) return false;
    uint32_t mac_any = 0, addr_any = 0;
    for (uint32_t k = 0; k < 6; ++k) mac_any |= e->mac[k];
    for (uint32_t k = 0; k < 16; ++k) addr_any |= e->addr[k];
    if (!mac_any) return false;
    for (uint32_t k = 4; e->family == 4 && k < 16; ++k)
        if (e->addr[k]) return false;
    if (e->family == 6 && (e->addr[0] == 0xFFu || !addr_any)) return false;
    return true;
}

// The table, option, port and counter rules both device calls share.
bool common_ok(const void* d_umem, uint32_t opts, const xsk_gpu_neigh_entry* d_table, uint32_t n_entries, uint32_t n_ports,
               const uint64_t* d_bound, const xsk_gpu_neigh_stats* d_nstats) {
    if (!d_umem || (opts & ~XSK_GPU_OPT_MASK) || n_ports < 1u || n_ports > kNgMaxPorts) return false;
    if (n_entries > kNgMaxEntries || (n_entries && !d_table) || ((uintptr_t)d_table & 7u)) return false;
    return !((uintptr_t)d_bound & 7u) && !((uintptr_t)d_nstats & 7u);
}

bool neigh_ok(const void* d_umem, const xsk_gpu_desc* d_descs, const uint32_t* d_n, uint32_t n_max, uint32_t opts,
              const xsk_gpu_neigh_entry* d_table, uint32_t n_entries, uint32_t n_ports, const uint64_t* d_bound,
              const uint8_t* d_nverdicts, const uint8_t* d_nports, const uint32_t* d_reply_len,
              const xsk_gpu_neigh_stats* d_nstats) {
    if (!common_ok(d_umem, opts, d_table, n_entries, n_ports, d_bound, d_nstats)) return false;
    if (!d_descs || ((uintptr_t)d_descs & 15u) || !d_nverdicts || !d_nports || n_max > XSK_GPU_MAX_BATCH) return false;
    return !((uintptr_t)d_n & 3u) && !((uintptr_t)d_reply_len & 3u);
}

bool share(const xsk_gpu_ring_dev* a, const xsk_gpu_ring_dev* b) {
    return a->d_ring == b->d_ring || a->d_producer == b->d_producer || a->d_consumer == b->d_consumer;
}
bool serve_ring_ok(const xsk_gpu_ring_dev* r) {
    return ring_ok(r, 16u) && pk_packable((uint64_t)(uintptr_t)r->d_ring, r->size);
}

bool serve_ok(const void* d_umem, const xsk_gpu_ring_dev* stack, const xsk_gpu_ring_dev* tx, uint32_t n_ports,
              const xsk_gpu_ring_dev* up, uint32_t max, uint32_t opts, const xsk_gpu_neigh_entry* d_table,
              uint32_t n_entries, const uint64_t* d_bound, const xsk_gpu_neigh_stats* d_nstats,
              const xsk_gpu_neigh_result* d_res) {
    if (!common_ok(d_umem, opts, d_table, n_entries, n_ports, d_bound, d_nstats)) return false;
    if (max < 1u || max > kNgServeThreads || ((uintptr_t)d_res & 3u) || !tx) return false;
    if (!serve_ring_ok(stack) || !serve_ring_ok(up) || share(stack, up)) return false;
    for (uint32_t p = 0; p < n_ports; ++p) {
        if (!serve_ring_ok(tx + p) || share(tx + p, stack) || share(tx + p, up)) return false;
        for (uint32_t q = 0; q < p; ++q)
            if (share(tx + p, tx + q)) return false;
    }
    return true;
}

PackedRing pack(const xsk_gpu_ring_dev* r) {
    return pk_pack((uint64_t)(uintptr_t)r->d_producer, (uint64_t)(uintptr_t)r->d_consumer, (uint64_t)(uintptr_t)r->d_ring,
                   r->size);
}

// The launches; every argument has been checked.
int neigh_launch(void* d_umem, uint64_t umem_size, const xsk_gpu_desc* d_descs, const uint32_t* d_n, uint32_t n_max,
                 uint32_t opts, const xsk_gpu_neigh_entry* d_table, uint32_t n_entries, uint32_t n_ports,
                 const uint64_t* d_bound, uint8_t* d_nverdicts, uint8_t* d_nports, uint32_t* d_reply_len,
                 xsk_gpu_neigh_stats* d_nstats, hipStream_t s) {
    if (n_max == 0) return 0;
    const size_t lds = (size_t)n_entries * kNgEntryWords * sizeof(uint32_t);
    neigh_kernel<<<dim3(cp_nwg(n_max)), dim3(kNgFrames), lds, s>>>((uint8_t*)d_umem, umem_size, d_descs, d_n, n_max, opts,
                                                                   d_table, n_entries, n_ports, d_bound, d_nverdicts,
                                                                   d_nports, d_reply_len, d_nstats);
    HIP_TRY(hipGetLastError());
    return 0;
}

int serve_launch(const ServeArgs& a, hipStream_t s) {
    const size_t lds = (size_t)a.n_entries * kNgEntryWords * sizeof(uint32_t);
    neigh_serve_kernel<<<dim3(1), dim3(kNgServeThreads), lds, s>>>(a);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

// For xsk_responder.hip (xsk_gpu_internal.h): the serve call's rules, stated once, here.
extern "C" int xsk_gpu__serve_ok(const void* d_umem, const struct xsk_gpu_ring_dev* stack, const struct xsk_gpu_ring_dev* tx,
                                 uint32_t n_ports, const struct xsk_gpu_ring_dev* up, uint32_t max, uint32_t opts,
                                 const struct xsk_gpu_neigh_entry* d_table, uint32_t n_entries, const uint64_t* d_bound,
                                 const struct xsk_gpu_neigh_stats* d_nstats, const struct xsk_gpu_neigh_result* d_res) {
    return serve_ok(d_umem, stack, tx, n_ports, up, max, opts, d_table, n_entries, d_bound, d_nstats, d_res) ? 1 : 0;
}

extern "C" {

int xsk_gpu_neigh_table_prepare(struct xsk_gpu_neigh_entry* entries, uint32_t n) {
    if (n > kNgMaxEntries || (n && !entries)) return -EINVAL;
    for (uint32_t i = 0; i < n; ++i)
        if (!entry_ok(&entries[i])) return -EINVAL;
    if (n) qsort(entries, n, sizeof(*entries), entry_cmp);
    for (uint32_t i = 1; i < n; ++i)
        if (entry_cmp(&entries[i - 1], &entries[i]) == 0) return -EEXIST;
    return 0;
}

int xsk_gpu_neigh_dev(void* d_umem, uint64_t umem_size, const struct xsk_gpu_desc* d_descs, const uint32_t* d_n,
                      uint32_t n_max, uint32_t opts, const struct xsk_gpu_neigh_entry* d_table, uint32_t n_entries,
                      uint32_t n_ports, const uint64_t* d_bound, uint8_t* d_nverdicts, uint8_t* d_nports,
                      uint32_t* d_reply_len, struct xsk_gpu_neigh_stats* d_nstats, void* stream) {
    if (!neigh_ok(d_umem, d_descs, d_n, n_max, opts, d_table, n_entries, n_ports, d_bound, d_nverdicts, d_nports,
                  d_reply_len, d_nstats))
        return -EINVAL;
    return neigh_launch(d_umem, umem_size, d_descs, d_n, n_max, opts, d_table, n_entries, n_ports, d_bound, d_nverdicts,
                        d_nports, d_reply_len, d_nstats, (hipStream_t)stream);
}

int xsk_gpu_neigh_serve_dev(void* d_umem, uint64_t umem_size, const struct xsk_gpu_ring_dev* stack,
                            const struct xsk_gpu_ring_dev* tx, uint32_t n_ports, const struct xsk_gpu_ring_dev* up,
                            uint32_t max, uint32_t opts, const struct xsk_gpu_neigh_entry* d_table, uint32_t n_entries,
                            const uint64_t* d_bound, struct xsk_gpu_neigh_stats* d_nstats,
                            struct xsk_gpu_neigh_result* d_res, void* stream) {
    if (!serve_ok(d_umem, stack, tx, n_ports, up, max, opts, d_table, n_entries, d_bound, d_nstats, d_res))
        return -EINVAL;
    ServeArgs a;
    for (uint32_t p = 0; p < kNgMaxPorts; ++p) a.ring[p] = p < n_ports ? pack(tx + p) : pk_pack(0u, 0u, 0u, 1u);
    a.ring[kNgUp] = pack(up);
    a.ring[kNgStack] = pack(stack);
    a.umem = (uint8_t*)d_umem;
    a.umem_size = umem_size;
    a.table = d_table;
    a.d_bound = d_bound;
    a.d_nstats = d_nstats;
    a.d_res = d_res;
    a.n_ports = n_ports;
    a.max = max;
    a.opts = opts;
    a.n_entries = n_entries;
    return serve_launch(a, (hipStream_t)stream);
}

}  // extern "C"
