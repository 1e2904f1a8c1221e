// xsk_steer.hip — xsk_gpu_steer_dev(): the ingress filter in front of up to 64 sockets (include/xsk_gpu.h; DESIGN.md
// §9.4).  The reference's XDP programs redirect through a 64-entry map (src/kern/inner_xdp.c:11-16,57-58; the devmap of
// src/kern/phy_xdp.c:8-12,67-80, whose key the code leaves at 0); here the key is the frame's IP destination address,
// looked up in a sorted table of at most 1024 entries, and the REDIRECT descriptors leave as a stable partition by
// port.  xsk_gpu_ingress_steer_dev() puts the indirect-count transform behind it on the same stream.
//
// Three launches, the compaction core (xsk_compact.h) with a port dimension; the decision and every index in
// xsk_steer.h (host and device).  All HBM / latency bound, no MFMA:
//   1. classify: the table staged once per workgroup into LDS as big-endian dwords (at most 24 KiB, dynamic: none with
//      an empty table), a lane per frame -- descriptor, the filter's two round trips with the destination riding in
//      them, binary search in LDS, port rule; per-workgroup, per-port counts into a port-major matrix;
//   2. scan: a 1024-thread workgroup per port, the exclusive scan of that port's row of the matrix; the row's total
//      rides in the cell [p][0], whose own value is always 0;
//   3. scatter: a lane per frame again; wave 0 of every workgroup turns the n_ports totals into the ports' first slots
//      (workgroup 0 writes them out: d_off); the rank among the wave's frames of the same port from one ballot per
//      distinct port in the wave, so batch order holds within a port and no atomic hands out a slot.
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/xsk_gpu.h"
#include "xsk_hip_util.h"
#include "xsk_steer.h"

using namespace xskgpu;

static_assert(sizeof(xsk_gpu_steer_entry) == 24 && kStEntryWords * 4 == 24, "an entry is staged dword for dword");
static_assert(sizeof(xsk_gpu_desc) == 16, "one 16-B load and store per descriptor");
static_assert(kStMaxPorts == kStWave && kStMaxPorts <= kStFrames, "a thread per port writes the workgroup's counts");

namespace {

typedef unsigned long long u64;

// (wave_ranks: the wave's frames by port, one ballot per distinct port present -- xsk_steer.h)

// ---- stage 1 ----
__global__ __launch_bounds__(kStFrames) void steer_classify_kernel(
    const uint8_t* __restrict__ umem, uint64_t umem_size, const xsk_gpu_desc* __restrict__ descs, uint32_t n,
    uint32_t opts, const xsk_gpu_steer_entry* __restrict__ table, uint32_t n_entries, uint32_t default_port,
    uint32_t n_ports, const uint64_t* __restrict__ d_bound, uint8_t* __restrict__ actions, uint8_t* __restrict__ ports,
    uint32_t* __restrict__ count, uint32_t nwg) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_tab[];  // n_entries staged entries
    __shared__ uint32_t s_cnt[kStWaves][kStMaxPorts];
    const uint32_t t = threadIdx.x;
    for (uint32_t k = t; k < n_entries; k += kStFrames) st_stage_entry(table + k, s_tab + k * kStEntryWords);
    (&s_cnt[0][0])[t] = 0u;  // kStWaves * kStMaxPorts == kStFrames
    const u64 bound = d_bound ? *d_bound : ~0ull;  // a uniform address: one scalar load
    __syncthreads();
    const uint32_t i = blockIdx.x * kStFrames + t;
    StVerdict v = {0u, kStPass};
    if (i < n) {
        v = st_steer_one(umem, umem_size, descs[i], opts, s_tab, n_entries, default_port, n_ports, bound);
        actions[i] = (uint8_t)v.act;
        ports[i] = (uint8_t)v.port;
    }
    if (!count) return;  // actions and ports only (uniform)
    wave_ranks(v.act == XSK_GPU_XDP_REDIRECT, v.port, s_cnt);
    __syncthreads();
    if (t < n_ports) count[st_cell(t, blockIdx.x, nwg)] = s_cnt[0][t] + s_cnt[1][t] + s_cnt[2][t] + s_cnt[3][t];
}
static_assert(kStWaves == 4 && kStWaves * kStMaxPorts == kStFrames, "the sums and the zeroing above");

// ---- stage 2: a workgroup per port scans that port's row of the matrix in place, exclusive (thread t owns a
// contiguous run of the row's cells: cp_scan_cells).  The exclusive value of the cell [p][0] is always 0, so
// that cell carries the row's total instead: stage 3 turns the n_ports totals into d_off ----
__global__ __launch_bounds__(kStScanThreads) void steer_scan_kernel(uint32_t* __restrict__ count, uint32_t nwg) {
    __shared__ uint32_t s[kStScanThreads];
    uint32_t* __restrict__ row = count + st_cell(blockIdx.x, 0u, nwg);
    uint32_t b, e;
    cp_scan_run(nwg, threadIdx.x, &b, &e);
    cp_scan_cells(row, b, e, s, st_scanned_cell);
}

// ---- stage 3 ----
__global__ __launch_bounds__(kStFrames) void steer_scatter_kernel(const xsk_gpu_desc* __restrict__ descs, uint32_t n,
                                                                  const uint8_t* __restrict__ actions,
                                                                  const uint8_t* __restrict__ ports,
                                                                  const uint32_t* __restrict__ cell_off, uint32_t nwg,
                                                                  uint32_t n_ports, xsk_gpu_desc* __restrict__ out,
                                                                  uint32_t* __restrict__ d_off) {
    __shared__ uint32_t s_cnt[kStWaves][kStMaxPorts];
    __shared__ uint32_t s_base[kStMaxPorts];
    const uint32_t t = threadIdx.x, i = blockIdx.x * kStFrames + t;
    (&s_cnt[0][0])[t] = 0u;
    if (t < kStWave) {  // wave 0, a lane per port: the rows' totals -> the ports' first slots; workgroup 0 writes d_off
        const uint32_t tot = t < n_ports ? cell_off[st_cell(t, 0u, nwg)] : 0u;
        uint32_t inc = tot;
        for (uint32_t o = 1; o < kStWave; o <<= 1) {
            const uint32_t v = __shfl_up(inc, o, kStWave);
            inc += t >= o ? v : 0u;
        }
        s_base[t] = inc - tot;
        if (blockIdx.x == 0u) {
            if (t < n_ports) d_off[t] = inc - tot;
            if (t == n_ports - 1u) d_off[n_ports] = inc;
        }
    }
    bool r = false;
    uint32_t port = 0;
    uint4 d = make_uint4(0u, 0u, 0u, 0u);
    if (i < n) {
        r = actions[i] == XSK_GPU_XDP_REDIRECT;
        port = ports[i] & (kStMaxPorts - 1u);  // (a REDIRECT frame's port is below n_ports <= 64)
        d = reinterpret_cast<const uint4*>(descs)[i];
    }
    __syncthreads();
    const uint32_t rank = wave_ranks(r, port, s_cnt);
    __syncthreads();
    if (r) {
        uint32_t lower = 0;
        for (uint32_t k = 0; k < kStWaves; ++k) lower += k < cp_wave() ? s_cnt[k][port] : 0u;
        const uint32_t in_row = st_cell_offset(blockIdx.x, cell_off[st_cell(port, blockIdx.x, nwg)]);
        reinterpret_cast<uint4*>(out)[st_slot(s_base[port], in_row, lower, rank)] = d;
    }
}

int entry_cmp(const void* a, const void* b) {
    const xsk_gpu_steer_entry* x = (const xsk_gpu_steer_entry*)a;
    const xsk_gpu_steer_entry* y = (const xsk_gpu_steer_entry*)b;
    if (x->family != y->family) return x->family < y->family ? -1 : 1;
    return memcmp(x->addr, y->addr, 16);
}

bool steer_args_ok(const void* d_umem, const struct xsk_gpu_desc* d_descs, uint32_t n, uint32_t opts,
                   const struct xsk_gpu_steer_entry* d_table, uint32_t n_entries, uint32_t default_port,
                   uint32_t n_ports, const uint64_t* d_bound, uint8_t* d_actions, uint8_t* d_ports,
                   struct xsk_gpu_desc* d_out, uint32_t* d_off, void* d_workspace) {
    if (opts & ~XSK_GPU_OPT_MASK) return false;
    // the filter's rules (xsk_classify.hip), d_off in the place of d_nout
    if (!d_umem || !d_descs || !d_actions || !d_workspace || (d_out && !d_off) || ((uintptr_t)d_descs & 15u) ||
        ((uintptr_t)d_out & 15u) || n > XSK_GPU_MAX_BATCH)
        return false;
    if (n_ports < 1u || n_ports > kStMaxPorts || (default_port >= n_ports && default_port != kStPass)) return false;
    if (n_entries > kStMaxEntries || (n_entries && (!d_table || ((uintptr_t)d_table & 7u)))) return false;
    if (((uintptr_t)d_bound & 7u) || ((uintptr_t)d_off & 3u) || !d_ports || (d_off && !d_out)) return false;
    return true;
}

// The launches; every argument has been checked.
int steer_launch(const void* d_umem, uint64_t umem_size, const struct xsk_gpu_desc* d_descs, uint32_t n, uint32_t opts,
                 const struct xsk_gpu_steer_entry* d_table, uint32_t n_entries, uint32_t default_port, uint32_t n_ports,
                 const uint64_t* d_bound, uint8_t* d_actions, uint8_t* d_ports, struct xsk_gpu_desc* d_out,
                 uint32_t* d_off, void* d_workspace, void* stream) {
    const hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        if (d_off) HIP_TRY(hipMemsetAsync(d_off, 0, (size_t)(n_ports + 1u) * sizeof(uint32_t), s));
        return 0;
    }
    const uint32_t nwg = cp_nwg(n);
    uint32_t* cells = (uint32_t*)d_workspace;
    const size_t lds = (size_t)n_entries * kStEntryWords * sizeof(uint32_t);
    steer_classify_kernel<<<dim3(nwg), dim3(kStFrames), lds, s>>>((const uint8_t*)d_umem, umem_size, d_descs, n, opts,
                                                                  d_table, n_entries, default_port, n_ports, d_bound,
                                                                  d_actions, d_ports, d_out ? cells : nullptr, nwg);
    HIP_TRY(hipGetLastError());
    if (d_out) {
        steer_scan_kernel<<<dim3(n_ports), dim3(kStScanThreads), 0, s>>>(cells, nwg);
        HIP_TRY(hipGetLastError());
        steer_scatter_kernel<<<dim3(nwg), dim3(kStFrames), 0, s>>>(d_descs, n, (const uint8_t*)d_actions,
                                                                   (const uint8_t*)d_ports, (const uint32_t*)cells, nwg,
                                                                   n_ports, d_out, d_off);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

}  // namespace

extern "C" {

int xsk_gpu_steer_table_prepare(struct xsk_gpu_steer_entry* entries, uint32_t n) {
    if (n > kStMaxEntries || (n && !entries)) return -EINVAL;
    for (uint32_t i = 0; i < n; ++i) {
        const xsk_gpu_steer_entry* e = &entries[i];
        if ((e->family != 4 && e->family != 6) || e->port >= kStMaxPorts) return -EINVAL;
        for (uint32_t k = 0; k < 6; ++k)
            if (e->pad[k]) return -EINVAL;
        for (uint32_t k = 4; e->family == 4 && k < 16; ++k)
            if (e->addr[k]) return -EINVAL;
    }
    if (n) qsort(entries, n, sizeof(*entries), entry_cmp);
    for (uint32_t i = 1; i < n; ++i)
        if (entry_cmp(&entries[i - 1], &entries[i]) == 0) return -EEXIST;
    return 0;
}

size_t xsk_gpu_steer_workspace_size(uint32_t n, uint32_t n_ports) {
    if (n_ports > kStMaxPorts) n_ports = kStMaxPorts;
    return st_workspace_bytes(n, n_ports);
}

int xsk_gpu_steer_dev(const void* d_umem, uint64_t umem_size, const struct xsk_gpu_desc* d_descs, uint32_t n,
                      uint32_t opts, const struct xsk_gpu_steer_entry* d_table, uint32_t n_entries,
                      uint32_t default_port, uint32_t n_ports, const uint64_t* d_bound, uint8_t* d_actions,
                      uint8_t* d_ports, struct xsk_gpu_desc* d_out, uint32_t* d_off, void* d_workspace, void* stream) {
    if (!steer_args_ok(d_umem, d_descs, n, opts, d_table, n_entries, default_port, n_ports, d_bound, d_actions, d_ports,
                       d_out, d_off, d_workspace))
        return -EINVAL;
    return steer_launch(d_umem, umem_size, d_descs, n, opts, d_table, n_entries, default_port, n_ports, d_bound,
                        d_actions, d_ports, d_out, d_off, d_workspace, stream);
}

int xsk_gpu_ingress_steer_dev(void* d_umem, uint64_t umem_size, const struct xsk_gpu_desc* d_descs, uint32_t n,
                              uint32_t opts, const struct xsk_gpu_steer_entry* d_table, uint32_t n_entries,
                              uint32_t default_port, uint32_t n_ports, const uint64_t* d_bound, uint8_t* d_actions,
                              uint8_t* d_ports, struct xsk_gpu_desc* d_out, uint32_t* d_off, uint8_t* d_verdicts,
                              struct xsk_gpu_rec* d_recs, struct xsk_gpu_stats* d_stats, void* d_workspace,
                              void* stream) {
    if (!d_out || !d_off || !steer_args_ok(d_umem, d_descs, n, opts, d_table, n_entries, default_port, n_ports, d_bound,
                                           d_actions, d_ports, d_out, d_off, d_workspace))
        return -EINVAL;
    // the transform's rules over d_out: with a bound of 0 frames xsk_gpu_echo_dev_indirect() checks every argument and
    // returns without a device call (include/xsk_gpu.h)
    const uint32_t* d_total = d_off + n_ports;
    int rc = xsk_gpu_echo_dev_indirect(d_umem, umem_size, d_out, d_total, 0, opts, d_verdicts, d_recs, d_stats, stream);
    if (rc) return rc;
    rc = steer_launch(d_umem, umem_size, d_descs, n, opts, d_table, n_entries, default_port, n_ports, d_bound, d_actions,
                      d_ports, d_out, d_off, d_workspace, stream);
    if (rc || n == 0) return rc;  // (n == 0: d_off has been zeroed)
    return xsk_gpu_echo_dev_indirect(d_umem, umem_size, d_out, d_total, n, opts, d_verdicts, d_recs, d_stats, stream);
}

}  // extern "C"
