"""xsknet_amd — MI355X (gfx950) ICMP-echo frame transform behind a C ABI.

The product is ``libxsknet_amd.so`` (HIP kernels + C host code, see ``include/xsk_gpu.h``).  This
module is ctypes plumbing so tests and ``bench.py`` can drive that ABI with torch-allocated device
memory; it contains no compute and has no fallback: if the shared library is missing or cannot be
loaded, importing the bindings raises.

Reference path replaced: ``process_packet``/``csum_replace2`` in
``/root/reference/src/lib/xsk_receive.c:101-190`` called per descriptor from the RX batch loop
``xsk_receive.c:220-233``.
"""
from __future__ import annotations

import ctypes as C
import errno as _errno
import mmap
import os
from typing import Optional

import numpy as np

__all__ = [
    "LIB_PATH", "lib", "build_id", "XskGpuError", "DESC_DTYPE", "REC_DTYPE", "STATS_DTYPE", "VERDICTS",
    "TX_REPLY", "DROP_SHORT", "DROP_NOT_IPV4", "DROP_NOT_ICMP", "DROP_NOT_ECHO", "DROP_BAD_DESC",
    "echo_dev", "synth_dev", "rearm_dev", "stream_read_dev", "workspace_size", "EchoContext",
    "MODE_ZEROCOPY", "MODE_STAGED", "MODE_LOWLAT", "LOWLAT_MAX", "MultiContext", "tune_lib", "lowlat_reserve", "lowlat_cap", "timing_enable", "timing_read", "Ring", "FramePool", "RxResult",
    "classify_dev", "XDP_DROP", "XDP_PASS", "XDP_REDIRECT", "DROP_BAD_IP", "DROP_BAD_CSUM",
    "OPT_STRICT_IPV4", "OPT_VLAN", "OPT_VERIFY_CSUM", "OPT_ALL", "F_IP_CSUM_OK", "F_ICMP_CSUM_OK", "F_VLAN",
    "F_IP_OPTIONS", "OPT_IPV6", "OPT_MASK", "F_IPV6",
    "egress_dev", "egress_workspace_size", "EGRESS_COUNTS_DTYPE",
    "egress_ports_dev", "egress_ports_workspace_size",
    "STEER_ENTRY_DTYPE", "STEER_PASS", "STEER_MAX_PORTS", "STEER_MAX_ENTRIES", "steer_table_prepare",
    "steer_workspace_size", "steer_dev", "ingress_steer_dev",
    "RingDev", "PoolDev", "RxPlan", "rx_begin_dev", "rx_end_dev", "rx_step_dev", "rx_step_dev_workspace_size",
    "tx_complete_dev",
    "RxSteerResult", "rx_prepare_ports_dev", "rx_end_ports_dev", "rx_step_steer_dev", "rx_step_steer_dev_workspace_size",
    "RxPassResult", "rx_pass_end_dev", "rx_pass_step_dev", "rx_pass_step_dev_workspace_size",
    "COMPLETE_MAX_RINGS", "tx_complete_rings_dev", "rx_loop_dev", "rx_loop_fused_dev",
    "RX_MAX_QUEUES", "RxQueue", "rx_queue", "rx_queues_block_size", "rx_queues_prepare", "rx_queues_dev",
    "NEIGH_ENTRY_DTYPE", "NEIGH_STATS_DTYPE", "NEIGH_RESULT_DTYPE", "NEIGH_MAX_ENTRIES", "NEIGH_VERDICTS",
    "NEIGH_NONE", "NEIGH_ARP_REPLY", "NEIGH_NA_REPLY", "NEIGH_MALFORMED", "NEIGH_UNKNOWN", "NEIGH_UNBOUND", "NEIGH_LEFT",
    "neigh_table_prepare", "neigh_dev", "neigh_serve_dev",
    "ResponderQueue", "responder_queue", "responder_dev", "responder_block_size", "responder_prepare",
    "responder_queues_dev",
    "UNREACH_STATS_DTYPE", "UNREACH_RESULT_DTYPE", "UNREACH_VERDICTS", "UNREACH_OPEN_BYTES",
    "UNREACH_NONE", "UNREACH_UNREACH4", "UNREACH_UNREACH6", "UNREACH_MALFORMED", "UNREACH_UNKNOWN", "UNREACH_UNBOUND",
    "UNREACH_LEFT", "UNREACH_NO_ROOM", "UNREACH_LIMITED", "unreach_dev", "unreach_serve_dev",
]

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libxsknet_amd.so")
# the product kernel at alternative switch values for in-process A/B (tools/abbench.py) and its parity tests; never
# the product path
TUNE_LIB_PATH = os.path.join(_HERE, "libxsknet_amd_tune.so")

TX_REPLY, DROP_SHORT, DROP_NOT_IPV4, DROP_NOT_ICMP, DROP_NOT_ECHO, DROP_BAD_DESC, DROP_BAD_IP, DROP_BAD_CSUM = range(8)
VERDICTS = ["TX_REPLY", "DROP_SHORT", "DROP_NOT_IPV4", "DROP_NOT_ICMP", "DROP_NOT_ECHO", "DROP_BAD_DESC",
            "DROP_BAD_IP", "DROP_BAD_CSUM"]
# wire-format options (include/xsk_gpu.h XSK_GPU_OPT_*) and record flags
OPT_STRICT_IPV4, OPT_VLAN, OPT_VERIFY_CSUM, OPT_ALL = 1, 2, 4, 7
OPT_IPV6, OPT_MASK = 0x10, 0x17  # ICMPv6 echo too; every valid bit (0x8 is reserved)
F_IP_CSUM_OK, F_ICMP_CSUM_OK, F_VLAN, F_IP_OPTIONS, F_IPV6 = 1, 2, 4, 8, 0x10
MODE_ZEROCOPY, MODE_STAGED, MODE_LOWLAT = 0, 1, 2
LOWLAT_MAX = 1024  # XSK_GPU_LOWLAT_MAX
RX_PIPE_MAX = 8  # XSK_GPU_RX_PIPE_MAX
MULTI_MAX = 16  # XSK_GPU_MULTI_MAX
LOWLAT_PER_DEVICE = 8  # XSK_GPU_LOWLAT_PER_DEVICE (the cap is min(this, GPU_MAX_HW_QUEUES), 4 by default)

# struct xsk_gpu_desc == struct xdp_desc (linux/if_xdp.h)
DESC_DTYPE = np.dtype([("addr", "<u8"), ("len", "<u4"), ("options", "<u4")])
# struct xsk_gpu_rec (16 B)
REC_DTYPE = np.dtype([
    ("verdict", "u1"), ("flags", "u1"), ("ip_proto", "u1"), ("icmp_type", "u1"),
    ("icmp_code", "u1"), ("ip_vihl", "u1"), ("eth_proto", "<u2"), ("icmp_csum_in", "<u2"),
    ("icmp_csum_out", "<u2"), ("ip_sum", "<u2"), ("icmp_sum", "<u2"),
])
# struct xsk_gpu_stats == struct stats_record (xsk_utils.h:17-23)
STATS_DTYPE = np.dtype([("timestamp", "<u8"), ("rx_packets", "<u8"), ("rx_bytes", "<u8"),
                        ("tx_packets", "<u8"), ("tx_bytes", "<u8")])
# struct xsk_gpu_egress_counts (16 B, device memory): what egress_dev leaves beside its two lists
EGRESS_COUNTS_DTYPE = np.dtype([("n", "<u4"), ("n_tx", "<u4"), ("n_tx_full", "<u4"), ("n_free", "<u4")])
assert DESC_DTYPE.itemsize == 16 and REC_DTYPE.itemsize == 16 and STATS_DTYPE.itemsize == 40
assert EGRESS_COUNTS_DTYPE.itemsize == 16
# struct xsk_gpu_steer_entry (24 B): one row of steer_dev's table, key (family, addr) -> port
STEER_ENTRY_DTYPE = np.dtype([("addr", "u1", (16,)), ("family", "u1"), ("port", "u1"), ("pad", "u1", (6,))])
STEER_PASS, STEER_MAX_PORTS, STEER_MAX_ENTRIES = 0xFF, 64, 1024  # XSK_GPU_STEER_*
assert STEER_ENTRY_DTYPE.itemsize == 24
COMPLETE_MAX_RINGS = STEER_MAX_PORTS + 1  # XSK_GPU_COMPLETE_MAX_RINGS: a completion ring per port, and the stack's
RX_MAX_QUEUES = 1024  # XSK_GPU_RX_MAX_QUEUES: the queues of one rx_queues_dev call
# struct xsk_gpu_neigh_entry (24 B): one row of the neighbour responder's table, key (family, addr) -> port, mac
NEIGH_ENTRY_DTYPE = np.dtype([("addr", "u1", (16,)), ("family", "u1"), ("port", "u1"), ("mac", "u1", (6,))])
# struct xsk_gpu_neigh_stats (32 B, accumulated) and struct xsk_gpu_neigh_result (32 B, written)
NEIGH_STATS_DTYPE = np.dtype([("seen", "<u8"), ("arp_replies", "<u8"), ("na_replies", "<u8"), ("reply_bytes", "<u8")])
NEIGH_RESULT_DTYPE = np.dtype([("consumed", "<u4"), ("arp_replies", "<u4"), ("na_replies", "<u4"), ("up", "<u4"),
                               ("backlog", "<u4"), ("reserved", "<u4", (3,))])
assert NEIGH_ENTRY_DTYPE.itemsize == 24 and NEIGH_STATS_DTYPE.itemsize == 32 and NEIGH_RESULT_DTYPE.itemsize == 32
NEIGH_MAX_ENTRIES = 1024  # XSK_GPU_NEIGH_MAX_ENTRIES
# enum xsk_gpu_neigh_verdict
NEIGH_NONE, NEIGH_ARP_REPLY, NEIGH_NA_REPLY, NEIGH_MALFORMED, NEIGH_UNKNOWN, NEIGH_UNBOUND, NEIGH_LEFT = range(7)
NEIGH_VERDICTS = ["NONE", "ARP_REPLY", "NA_REPLY", "MALFORMED", "UNKNOWN", "UNBOUND", "LEFT"]
# struct xsk_gpu_unreach_stats (64 B, accumulated) and struct xsk_gpu_unreach_result (32 B, written)
UNREACH_STATS_DTYPE = np.dtype([("seen", "<u8"), ("unreach4", "<u8"), ("unreach6", "<u8"), ("reply_bytes", "<u8"),
                                ("limited", "<u8"), ("reserved", "<u8", (3,))])
UNREACH_RESULT_DTYPE = np.dtype([("consumed", "<u4"), ("unreach4", "<u4"), ("unreach6", "<u4"), ("rest", "<u4"),
                                 ("backlog", "<u4"), ("limited", "<u4"), ("reserved", "<u4", (2,))])
assert UNREACH_STATS_DTYPE.itemsize == 64 and UNREACH_RESULT_DTYPE.itemsize == 32
# enum xsk_gpu_unreach_verdict
(UNREACH_NONE, UNREACH_UNREACH4, UNREACH_UNREACH6, UNREACH_MALFORMED, UNREACH_UNKNOWN, UNREACH_UNBOUND, UNREACH_LEFT,
 UNREACH_NO_ROOM, UNREACH_LIMITED) = range(9)
UNREACH_VERDICTS = ["NONE", "UNREACH4", "UNREACH6", "MALFORMED", "UNKNOWN", "UNBOUND", "LEFT", "NO_ROOM", "LIMITED"]
UNREACH_OPEN_BYTES = 8192  # the open-port map: a bit per UDP port


class XskGpuError(RuntimeError):
    def __init__(self, fn: str, rc: int):
        name = _errno.errorcode.get(-rc, str(rc))
        detail = ""
        if _lib is not None:
            detail = f" (last HIP error: {_lib.xsk_gpu_last_error().decode()})"
        super().__init__(f"{fn} failed: -{name}{detail}")
        self.rc = rc


class Ring(C.Structure):
    """struct xsk_gpu_ring == libxdp's struct xsk_ring_prod / xsk_ring_cons."""
    _fields_ = [("cached_prod", C.c_uint32), ("cached_cons", C.c_uint32), ("mask", C.c_uint32),
                ("size", C.c_uint32), ("producer", C.c_void_p), ("consumer", C.c_void_p), ("ring", C.c_void_p),
                ("flags", C.c_void_p)]


class FramePool(C.Structure):
    """struct xsk_gpu_frame_pool: the client's free-frame stack (xsk_utils.h:30-31)."""
    _fields_ = [("addr", C.c_void_p), ("n_free", C.c_uint32), ("capacity", C.c_uint32)]


class RxResult(C.Structure):
    _fields_ = [("received", C.c_uint32), ("replied", C.c_uint32), ("tx_full", C.c_uint32),
                ("refilled", C.c_uint32)]


assert C.sizeof(Ring) == 48 and C.sizeof(FramePool) == 16 and C.sizeof(RxResult) == 16


class RingDev(C.Structure):
    """struct xsk_gpu_ring_dev: a ring whose index words and entries live in device memory (the struct itself is host
    memory, read when a call is made)."""
    _fields_ = [("d_producer", C.c_void_p), ("d_consumer", C.c_void_p), ("d_ring", C.c_void_p), ("size", C.c_uint32),
                ("reserved", C.c_uint32)]

    @classmethod
    def of(cls, producer, consumer, ring, size: int) -> "RingDev":
        """From torch device tensors: two uint32 words (int32 tensors of one element) and the entry array."""
        return cls(_ptr(producer), _ptr(consumer), _ptr(ring), size, 0)


class PoolDev(C.Structure):
    """struct xsk_gpu_pool_dev: struct xsk_gpu_frame_pool with the stack and its count in device memory."""
    _fields_ = [("d_addr", C.c_void_p), ("d_n_free", C.c_void_p), ("capacity", C.c_uint32), ("reserved", C.c_uint32)]

    @classmethod
    def of(cls, addr, n_free, capacity: int) -> "PoolDev":
        return cls(_ptr(addr), _ptr(n_free), capacity, 0)


class RxPlan(C.Structure):
    """struct xsk_gpu_rx_plan (device memory): what rx_begin_dev decided."""
    _fields_ = [("received", C.c_uint32), ("tx_room", C.c_uint32), ("refilled", C.c_uint32), ("rx_cons", C.c_uint32),
                ("fq_prod", C.c_uint32), ("pool_n", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class RxSteerResult(C.Structure):
    """struct xsk_gpu_rx_steer_result (device memory): what rx_end_ports_dev / rx_step_steer_dev leave."""
    _fields_ = [("received", C.c_uint32), ("redirected", C.c_uint32), ("replied", C.c_uint32), ("tx_full", C.c_uint32),
                ("refilled", C.c_uint32), ("freed", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class RxPassResult(C.Structure):
    """struct xsk_gpu_rx_pass_result (device memory): what rx_pass_end_dev / rx_pass_step_dev leave."""
    _fields_ = [("received", C.c_uint32), ("redirected", C.c_uint32), ("replied", C.c_uint32), ("tx_full", C.c_uint32),
                ("refilled", C.c_uint32), ("freed", C.c_uint32), ("passed", C.c_uint32), ("pass_full", C.c_uint32)]


assert C.sizeof(RingDev) == 32 and C.sizeof(PoolDev) == 24 and C.sizeof(RxPlan) == 32 and C.sizeof(RxSteerResult) == 32
assert C.sizeof(RxPassResult) == 32


class RxQueue(C.Structure):
    """struct xsk_gpu_rx_queue (host memory): one queue's arguments of xsk_gpu_rx_fused_loop_dev, for
    rx_queues_prepare.  rx_queue() builds one from rx_loop_fused_dev's arguments and keeps what it points to alive."""
    _fields_ = [("d_umem", C.c_void_p), ("umem_size", C.c_uint64), ("rx", C.POINTER(RingDev)),
                ("fill", C.POINTER(RingDev)), ("tx", C.POINTER(RingDev)), ("stack", C.POINTER(RingDev)),
                ("pool", C.POINTER(PoolDev)), ("d_table", C.c_void_p), ("d_bound", C.c_void_p),
                ("d_actions", C.c_void_p), ("d_ports", C.c_void_p), ("d_port_counts", C.c_void_p),
                ("d_stats", C.c_void_p), ("d_port_stats", C.c_void_p), ("d_res", C.c_void_p),
                ("comp", C.POINTER(RingDev)), ("d_moved", C.c_void_p), ("d_pushed", C.c_void_p),
                ("d_workspace", C.c_void_p), ("max_batch", C.c_uint32), ("n_ports", C.c_uint32),
                ("n_entries", C.c_uint32), ("default_port", C.c_uint32), ("n_comp", C.c_uint32),
                ("complete_max", C.c_uint32)]


assert C.sizeof(RxQueue) == 176


class ResponderQueue(C.Structure):
    """struct xsk_gpu_responder_queue (host memory): one queue's arguments of xsk_gpu_responder_dev -- the fused call's
    (q, with q.stack required) and the serve call's up, table, counters, result and bound.  responder_queue() builds one."""
    _fields_ = [("q", RxQueue), ("up", C.POINTER(RingDev)), ("d_ntable", C.c_void_p), ("d_nstats", C.c_void_p),
                ("d_nres", C.c_void_p), ("n_nentries", C.c_uint32), ("serve_max", C.c_uint32)]


assert C.sizeof(ResponderQueue) == 216

_lib: Optional[C.CDLL] = None

_P = C.c_void_p
_SIGS = {
    "xsk_gpu_abi_version": ([], C.c_int),
    "xsk_gpu_last_error": ([], C.c_char_p),
    "xsk_gpu_build_id": ([], C.c_char_p),
    "xsk_gpu_workspace_size": ([C.c_int, C.c_uint32], C.c_size_t),
    "xsk_gpu_echo_dev": ([_P, C.c_uint64, _P, C.c_uint32, _P, _P, _P, _P, _P], C.c_int),
    "xsk_gpu_echo_dev_opts": ([_P, C.c_uint64, _P, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P], C.c_int),
    "xsk_gpu_echo_dev_indirect": ([_P, C.c_uint64, _P, _P, C.c_uint32, C.c_uint32, _P, _P, _P, _P], C.c_int),
    "xsk_gpu_ingress_dev_opts": ([_P, C.c_uint64, _P, C.c_uint32, C.c_uint32, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P],
                                 C.c_int),
    "xsk_gpu_egress_workspace_size": ([C.c_uint32], C.c_size_t),
    "xsk_gpu_egress_dev": ([_P, _P, _P, C.c_uint32, _P, _P, _P, _P, _P, _P, _P], C.c_int),
    "xsk_gpu_egress_ports_workspace_size": ([C.c_uint32, C.c_uint32], C.c_size_t),
    "xsk_gpu_egress_ports_dev": ([_P, _P, _P, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P, _P, _P, _P], C.c_int),
    "xsk_gpu_steer_table_prepare": ([_P, C.c_uint32], C.c_int),
    "xsk_gpu_steer_workspace_size": ([C.c_uint32, C.c_uint32], C.c_size_t),
    "xsk_gpu_steer_dev": ([_P, C.c_uint64, _P, C.c_uint32, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, _P,
                           _P, _P, _P, _P], C.c_int),
    "xsk_gpu_ingress_steer_dev": ([_P, C.c_uint64, _P, C.c_uint32, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P,
                                   _P, _P, _P, _P, _P, _P, _P, _P, _P], C.c_int),
    "xsk_gpu_set_options": ([_P, C.c_uint32], C.c_int),
    "xsk_gpu_init": ([C.POINTER(_P), C.c_int, _P, C.c_uint64, C.c_uint32, C.c_int], C.c_int),
    "xsk_gpu_process": ([_P, _P, C.c_uint32, _P, _P, _P], C.c_int),
    "xsk_gpu_fini": ([_P], None),
    "xsk_gpu_ctx_mode": ([_P], C.c_int),
    "xsk_gpu_synth_dev": ([_P, C.c_uint64, _P, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                           C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, _P], C.c_int),
    "xsk_gpu_rearm_dev": ([_P, _P, _P, C.c_uint32, _P], C.c_int),
    "xsk_gpu_stream_read_dev": ([_P, C.c_uint64, _P, _P], C.c_int),
    "xsk_gpu_timing_enable": ([C.c_int], C.c_int),
    "xsk_gpu_timing_read": ([C.POINTER(C.c_double), C.POINTER(C.c_uint64)], C.c_int),
    "xsk_gpu_rx_step": ([_P, C.POINTER(Ring), C.POINTER(Ring), C.POINTER(Ring), C.POINTER(FramePool), C.c_uint32,
                         _P, C.POINTER(RxResult)], C.c_int),
    "xsk_gpu_tx_complete": ([C.POINTER(Ring), C.POINTER(FramePool), C.c_uint32], C.c_uint32),
    "xsk_gpu_rx_step_dev_workspace_size": ([C.c_uint32], C.c_size_t),
    "xsk_gpu_rx_begin_dev": ([C.POINTER(RingDev), C.POINTER(RingDev), C.POINTER(RingDev), C.POINTER(PoolDev), C.c_uint32,
                              _P, _P, _P], C.c_int),
    "xsk_gpu_rx_end_dev": ([C.POINTER(RingDev), C.POINTER(RingDev), C.POINTER(PoolDev), _P, _P, _P, _P, C.c_uint32, _P,
                            _P], C.c_int),
    "xsk_gpu_rx_step_dev": ([_P, C.c_uint64, C.POINTER(RingDev), C.POINTER(RingDev), C.POINTER(RingDev),
                             C.POINTER(PoolDev), C.c_uint32, C.c_uint32, _P, _P, _P, _P], C.c_int),
    "xsk_gpu_tx_complete_dev": ([C.POINTER(RingDev), C.POINTER(PoolDev), C.c_uint32, _P, _P], C.c_int),
    "xsk_gpu_rx_step_steer_dev_workspace_size": ([C.c_uint32, C.c_uint32], C.c_size_t),
    "xsk_gpu_rx_prepare_ports_dev": ([C.POINTER(RingDev), C.c_uint32, _P, _P, C.c_uint32, _P, _P], C.c_int),
    "xsk_gpu_rx_ports_end_dev": ([C.POINTER(RingDev), C.POINTER(RingDev), C.c_uint32, C.POINTER(PoolDev), _P, _P, _P, _P,
                                  _P, _P, _P, C.c_uint32, _P, _P, _P], C.c_int),
    "xsk_gpu_rx_step_steer_dev": ([_P, C.c_uint64, C.POINTER(RingDev), C.POINTER(RingDev), C.POINTER(RingDev),
                                   C.POINTER(PoolDev), C.c_uint32, C.c_uint32, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P,
                                   _P, _P, _P, _P, _P, _P, _P, _P], C.c_int),
    "xsk_gpu_rx_pass_step_dev_workspace_size": ([C.c_uint32, C.c_uint32], C.c_size_t),
    "xsk_gpu_rx_pass_end_dev": ([C.POINTER(RingDev), C.POINTER(RingDev), C.c_uint32, C.POINTER(RingDev),
                                 C.POINTER(PoolDev), _P, _P, _P, _P, _P, _P, _P, C.c_uint32, _P, _P, _P], C.c_int),
    "xsk_gpu_rx_pass_step_dev": ([_P, C.c_uint64, C.POINTER(RingDev), C.POINTER(RingDev), C.POINTER(RingDev),
                                  C.POINTER(RingDev), C.POINTER(PoolDev), C.c_uint32, C.c_uint32, _P, C.c_uint32,
                                  C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P, _P, _P, _P, _P], C.c_int),
    "xsk_gpu_tx_complete_rings_dev": ([C.POINTER(RingDev), C.c_uint32, C.POINTER(PoolDev), C.c_uint32, _P, _P, _P],
                                      C.c_int),
    "xsk_gpu_rx_loop_dev": ([_P, C.c_uint64, C.POINTER(RingDev), C.POINTER(RingDev), C.POINTER(RingDev),
                             C.POINTER(RingDev), C.POINTER(PoolDev), C.c_uint32, C.c_uint32, _P, C.c_uint32, C.c_uint32,
                             C.c_uint32, _P, _P, _P, _P, _P, _P, _P, C.POINTER(RingDev), C.c_uint32, C.c_uint32, _P, _P,
                             _P, _P], C.c_int),
    "xsk_gpu_rx_fused_loop_dev": ([_P, C.c_uint64, C.POINTER(RingDev), C.POINTER(RingDev), C.POINTER(RingDev),
                                   C.POINTER(RingDev), C.POINTER(PoolDev), C.c_uint32, C.c_uint32, _P, C.c_uint32, C.c_uint32,
                                   C.c_uint32, _P, _P, _P, _P, _P, _P, _P, C.POINTER(RingDev), C.c_uint32, C.c_uint32, _P, _P,
                                   _P, _P], C.c_int),
    "xsk_gpu_rx_queues_block_size": ([C.c_uint32], C.c_size_t),
    "xsk_gpu_rx_queues_prepare": ([C.POINTER(RxQueue), C.c_uint32, C.c_uint32, _P], C.c_int),
    "xsk_gpu_rx_queues_dev": ([_P, C.c_uint32, C.c_uint32, _P], C.c_int),
    "xsk_gpu_neigh_table_prepare": ([_P, C.c_uint32], C.c_int),
    "xsk_gpu_neigh_dev": ([_P, C.c_uint64, _P, _P, C.c_uint32, C.c_uint32, _P, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P,
                           _P], C.c_int),
    "xsk_gpu_responder_dev": ([C.POINTER(ResponderQueue), C.c_uint32, _P], C.c_int),
    "xsk_gpu_responder_block_size": ([C.c_uint32], C.c_size_t),
    "xsk_gpu_responder_prepare": ([C.POINTER(ResponderQueue), C.c_uint32, C.c_uint32, _P], C.c_int),
    "xsk_gpu_responder_queues_dev": ([_P, C.c_uint32, C.c_uint32, _P], C.c_int),
    "xsk_gpu_neigh_serve_dev": ([_P, C.c_uint64, C.POINTER(RingDev), C.POINTER(RingDev), C.c_uint32, C.POINTER(RingDev),
                                 C.c_uint32, C.c_uint32, _P, C.c_uint32, _P, _P, _P, _P], C.c_int),
    "xsk_gpu_unreach_dev": ([_P, C.c_uint64, _P, _P, C.c_uint32, C.c_uint32, _P, C.c_uint32, C.c_uint32, _P, _P, C.c_uint32,
                             _P, _P, _P, _P, _P], C.c_int),
    "xsk_gpu_unreach_serve_dev": ([_P, C.c_uint64, C.POINTER(RingDev), C.POINTER(RingDev), C.c_uint32, C.POINTER(RingDev),
                                   C.c_uint32, C.c_uint32, _P, C.c_uint32, _P, _P, C.c_uint32, _P, _P, _P, _P], C.c_int),
    "xsk_gpu_classify_workspace_size": ([C.c_uint32], C.c_size_t),
    "xsk_gpu_classify_dev": ([_P, C.c_uint64, _P, C.c_uint32, C.c_int, _P, _P, _P, _P, _P], C.c_int),
    "xsk_gpu_classify_dev_opts": ([_P, C.c_uint64, _P, C.c_uint32, C.c_uint32, C.c_int, _P, _P, _P, _P, _P], C.c_int),
    "xsk_gpu_multi_init": ([C.POINTER(_P), _P, C.c_uint32, _P, C.c_uint64, C.c_uint32, C.c_int], C.c_int),
    "xsk_gpu_multi_process": ([_P, _P, C.c_uint32, _P, _P, _P], C.c_int),
    "xsk_gpu_multi_set_options": ([_P, C.c_uint32], C.c_int),
    "xsk_gpu_multi_status": ([_P, _P, C.c_uint32], C.c_int),
    "xsk_gpu_stats_tx_failed": ([_P, _P, _P, _P, C.c_uint32], C.c_int),
    "xsk_gpu__multi_inject": ([_P, C.c_uint32, C.c_int], C.c_int),
    "xsk_gpu__lowlat_tune": ([_P, C.c_uint32, C.c_uint32, C.c_uint32], C.c_int),
    "xsk_gpu_multi_fini": ([_P], None),
    "xsk_gpu_lowlat_reserve": ([C.c_int, C.c_uint32], C.c_int),
    "xsk_gpu_lowlat_cap": ([C.c_int], C.c_int),
    "xsk_gpu__umem_refs": ([_P], C.c_int),
    "xsk_gpu__buf_kept": ([C.c_int], C.c_int),
    "xsk_gpu__staged_stats": ([_P, C.POINTER(C.c_uint64)], C.c_int),
    "xsk_gpu__staged_noalias": ([_P, C.c_uint32], C.c_int),
    "xsk_gpu__lowlat_outcomes": ([_P, C.POINTER(C.c_uint64)], C.c_int),
    "xsk_gpu__lowlat_served": ([_P, C.POINTER(C.c_uint64)], C.c_int),
    "xsk_gpu__lowlat_test_width": ([_P, C.c_uint32], C.c_int),
    "xsk_gpu__multi_ctx": ([_P, C.c_uint32], _P),
    "xsk_gpu__lowlat_live": ([C.c_int, C.POINTER(C.c_uint32)], C.c_int),
    "xsk_gpu__umem_view": ([_P, C.c_uint64, _P, C.c_uint64], C.c_int),
    "xsk_gpu_umem_alloc": ([C.POINTER(_P), C.c_uint64, C.POINTER(C.c_uint64)], C.c_int),
    "xsk_gpu_umem_free": ([_P, C.c_uint64], None),
    "xsk_gpu_rx_pipe_init": ([C.POINTER(_P), C.c_int, _P, C.c_uint64, C.c_uint32, C.c_int], C.c_int),
    "xsk_gpu_rx_pipe_step": ([_P, C.POINTER(Ring), C.POINTER(Ring), C.POINTER(Ring), C.POINTER(FramePool), C.c_uint32,
                              _P, C.POINTER(RxResult)], C.c_int),
    "xsk_gpu_rx_pipe_flush": ([_P, C.POINTER(Ring), C.POINTER(FramePool), _P, C.POINTER(RxResult)], C.c_int),
    "xsk_gpu_rx_pipe_set_options": ([_P, C.c_uint32], C.c_int),
    "xsk_gpu_rx_pipe_inflight": ([_P], C.c_uint32),
    "xsk_gpu_rx_pipe_depth": ([_P], C.c_uint32),
    "xsk_gpu_rx_pipe_fini": ([_P], None),
    "xsk_gpu__rx_pipe_ctx": ([_P, C.c_uint32], _P),
    # internal test / tool hook (xsk_gpu_internal.h): the product kernel with a forced workgroup count
    "xsk_gpu__echo_dev_grid": ([_P, C.c_uint64, _P, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P, C.c_uint32], C.c_int),
}
_TUNE_SIGS = {
    "xsk_gpu__product_variant": ([C.c_int, C.c_uint32, _P, C.c_uint64, _P, C.c_uint32, _P, _P, _P, _P], C.c_int),
}
_tune: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load libxsknet_amd.so (raises OSError if it is missing: there is no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError(f"{LIB_PATH} not built: run `make` (or __graft_entry__.build())")
        L = C.CDLL(LIB_PATH)
        for name, (args, res) in _SIGS.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = res
        _lib = L
    return _lib


def tune_lib() -> C.CDLL:
    """libxsknet_amd_tune.so: the product kernel at alternative switch values (tools/abbench.py, tests only)."""
    global _tune
    if _tune is None:
        lib()
        if not os.path.exists(TUNE_LIB_PATH):
            raise OSError(f"{TUNE_LIB_PATH} not built: run `make`")
        L = C.CDLL(TUNE_LIB_PATH)
        for name, (args, res) in _TUNE_SIGS.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = res
        _tune = L
    return _tune


def _check(fn: str, rc: int) -> None:
    if rc != 0:
        raise XskGpuError(fn, rc)


def _ptr(t) -> Optional[int]:
    """Device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    return t.data_ptr()


def _stream_ptr(stream) -> Optional[int]:
    if stream is None:
        import torch
        return torch.cuda.current_stream().cuda_stream
    return getattr(stream, "cuda_stream", stream)


def build_id() -> str:
    """xsk_gpu_build_id(): hash of the transform kernel's sources and flags in the loaded library."""
    return lib().xsk_gpu_build_id().decode()


def workspace_size(device: int, n: int) -> int:
    return int(lib().xsk_gpu_workspace_size(device, n))


def echo_dev(umem, descs, n: int, verdicts=None, recs=None, stats=None, workspace=None, stream=None,
             opts: int = 0, grid: int = 0) -> None:
    """xsk_gpu_echo_dev (opts == 0) / xsk_gpu_echo_dev_opts on torch device tensors (uint8 umem,
    uint8/int64 views of the structs).  grid != 0: the same product kernel with that many workgroups for a
    large batch (internal hook xsk_gpu__echo_dev_grid, tests only)."""
    if grid:
        _check("xsk_gpu__echo_dev_grid", lib().xsk_gpu__echo_dev_grid(
            _ptr(umem), umem.numel() * umem.element_size(), _ptr(descs), n, opts, _ptr(verdicts), _ptr(recs),
            _ptr(stats), _ptr(workspace), _stream_ptr(stream), grid))
        return
    if opts:
        _check("xsk_gpu_echo_dev_opts", lib().xsk_gpu_echo_dev_opts(
            _ptr(umem), umem.numel() * umem.element_size(), _ptr(descs), n, opts, _ptr(verdicts), _ptr(recs),
            _ptr(stats), _ptr(workspace), _stream_ptr(stream)))
        return
    _check("xsk_gpu_echo_dev", lib().xsk_gpu_echo_dev(
        _ptr(umem), umem.numel() * umem.element_size(), _ptr(descs), n, _ptr(verdicts), _ptr(recs), _ptr(stats),
        _ptr(workspace), _stream_ptr(stream)))


def echo_dev_indirect(umem, descs, count, n_max: int, verdicts=None, recs=None, stats=None, stream=None,
                      opts: int = 0) -> None:
    """xsk_gpu_echo_dev_indirect: the transform over the first min(count[0], n_max) descriptors, where `count` is a
    uint32 word on the device (an int32 tensor of one element) that the kernel reads when it executes."""
    _check("xsk_gpu_echo_dev_indirect", lib().xsk_gpu_echo_dev_indirect(
        _ptr(umem), umem.numel() * umem.element_size(), _ptr(descs), _ptr(count), n_max, opts, _ptr(verdicts),
        _ptr(recs), _ptr(stats), _stream_ptr(stream)))


XDP_DROP, XDP_PASS, XDP_REDIRECT = 1, 2, 4


def classify_dev(umem, descs, n: int, bound: bool, actions, out=None, nout=None, workspace=None, stream=None,
                 opts: int = 0) -> None:
    """xsk_gpu_classify_dev: the XDP ingress filter (inner_xdp.c:26-61) + in-order compaction.  Nonzero opts:
    xsk_gpu_classify_dev_opts, the VLAN- and IPv6-aware filter in front of echo_dev(opts=...)."""
    if workspace is None:
        import torch
        workspace = torch.empty(int(lib().xsk_gpu_classify_workspace_size(max(n, 1))), dtype=torch.uint8,
                                device=umem.device)
    if opts:
        _check("xsk_gpu_classify_dev_opts", lib().xsk_gpu_classify_dev_opts(
            _ptr(umem), umem.numel() * umem.element_size(), _ptr(descs), n, opts, 1 if bound else 0, _ptr(actions),
            _ptr(out), _ptr(nout), _ptr(workspace), _stream_ptr(stream)))
        return
    _check("xsk_gpu_classify_dev", lib().xsk_gpu_classify_dev(
        _ptr(umem), umem.numel() * umem.element_size(), _ptr(descs), n, 1 if bound else 0, _ptr(actions), _ptr(out),
        _ptr(nout), _ptr(workspace), _stream_ptr(stream)))


def ingress_dev(umem, descs, n: int, bound: bool, actions, out, nout, verdicts=None, recs=None, stats=None,
                workspace=None, stream=None, opts: int = 0) -> None:
    """xsk_gpu_ingress_dev_opts: classify_dev(opts) and, on the same stream, echo_dev_indirect(opts) over its
    compacted descriptors `out` and their count `nout`, with no host synchronisation between them.  Inside a graph
    capture pass `workspace` (classify_workspace_size bytes): allocating it here would be part of the capture."""
    if workspace is None:
        import torch
        workspace = torch.empty(int(lib().xsk_gpu_classify_workspace_size(max(n, 1))), dtype=torch.uint8,
                                device=umem.device)
    _check("xsk_gpu_ingress_dev_opts", lib().xsk_gpu_ingress_dev_opts(
        _ptr(umem), umem.numel() * umem.element_size(), _ptr(descs), n, opts, 1 if bound else 0, _ptr(actions),
        _ptr(out), _ptr(nout), _ptr(verdicts), _ptr(recs), _ptr(stats), _ptr(workspace), _stream_ptr(stream)))


def egress_workspace_size(n_max: int) -> int:
    """xsk_gpu_egress_workspace_size: bytes of device workspace egress_dev needs for a bound of n_max frames (0 up to
    LOWLAT_MAX)."""
    return int(lib().xsk_gpu_egress_workspace_size(n_max))


def egress_dev(descs, verdicts, n_max: int, tx, free, counts, count=None, tx_room=None, stats=None, workspace=None,
               stream=None) -> None:
    """xsk_gpu_egress_dev: (descriptors, verdicts) -> the TX descriptor list `tx`, the free-frame address list `free`
    (uint64 UMEM offsets) and `counts` (one EGRESS_COUNTS_DTYPE), all on the device, as xsk_gpu_rx_step's step 4 builds
    them.  `count` and `tx_room` are uint32 words on the device (int32 tensors of one element) that the kernels read
    when they execute: the frame count (None = n_max) and the TX ring's free slots (None = unlimited).  Behind
    ingress_dev: descs=out, count=nout.  Inside a graph capture pass `workspace` (egress_workspace_size bytes) when
    n_max > LOWLAT_MAX: allocating it here would be part of the capture."""
    if workspace is None and n_max > LOWLAT_MAX:
        import torch
        workspace = torch.empty(egress_workspace_size(n_max), dtype=torch.uint8, device=descs.device)
    _check("xsk_gpu_egress_dev", lib().xsk_gpu_egress_dev(
        _ptr(descs), _ptr(verdicts), _ptr(count), n_max, _ptr(tx_room), _ptr(tx), _ptr(free), _ptr(counts),
        _ptr(stats), _ptr(workspace), _stream_ptr(stream)))


def steer_table_prepare(entries: np.ndarray) -> np.ndarray:
    """xsk_gpu_steer_table_prepare on a copy of a host array of STEER_ENTRY_DTYPE: checked and sorted by (family,
    addr), the order steer_dev's search needs.  Raises XskGpuError (-EINVAL, -EEXIST)."""
    e = np.array(entries, dtype=STEER_ENTRY_DTYPE, copy=True).reshape(-1)
    _check("xsk_gpu_steer_table_prepare", lib().xsk_gpu_steer_table_prepare(e.ctypes.data if len(e) else None, len(e)))
    return e


def steer_workspace_size(n: int, n_ports: int) -> int:
    """xsk_gpu_steer_workspace_size: bytes of device workspace steer_dev needs for n frames and n_ports ports."""
    return int(lib().xsk_gpu_steer_workspace_size(n, n_ports))


def _steer_workspace(umem, n: int, n_ports: int):
    import torch
    return torch.empty(max(steer_workspace_size(max(n, 1), n_ports), 4), dtype=torch.uint8, device=umem.device)


def steer_dev(umem, descs, n: int, table, n_entries: int, default_port: int, n_ports: int, bound, actions, ports,
              out=None, off=None, workspace=None, stream=None, opts: int = 0) -> None:
    """xsk_gpu_steer_dev: the ingress filter with a port per REDIRECT frame, looked up by destination address in
    `table` (a device copy of a steer_table_prepare()d array, or None with n_entries == 0), and the REDIRECT
    descriptors in `out` grouped by port, port p's at out[off[p]:off[p + 1]] (`off`: n_ports + 1 uint32 words).
    `bound` is a uint64 word on the device (bit p = port p bound; None = all), read when the kernels execute.  Inside a
    graph capture pass `workspace` (steer_workspace_size bytes): allocating it here would be part of the capture."""
    if workspace is None:
        workspace = _steer_workspace(umem, n, n_ports)
    _check("xsk_gpu_steer_dev", lib().xsk_gpu_steer_dev(
        _ptr(umem), umem.numel() * umem.element_size(), _ptr(descs), n, opts, _ptr(table), n_entries, default_port,
        n_ports, _ptr(bound), _ptr(actions), _ptr(ports), _ptr(out), _ptr(off), _ptr(workspace), _stream_ptr(stream)))


def ingress_steer_dev(umem, descs, n: int, table, n_entries: int, default_port: int, n_ports: int, bound, actions,
                      ports, out, off, verdicts=None, recs=None, stats=None, workspace=None, stream=None,
                      opts: int = 0) -> None:
    """xsk_gpu_ingress_steer_dev: steer_dev(opts) and, on the same stream, echo_dev_indirect(opts) over `out` with the
    count off[n_ports]; verdicts and records are indexed by position in `out`, so port p's are
    verdicts[off[p]:off[p + 1]].  Inside a graph capture pass `workspace`, as for steer_dev."""
    if workspace is None:
        workspace = _steer_workspace(umem, n, n_ports)
    _check("xsk_gpu_ingress_steer_dev", lib().xsk_gpu_ingress_steer_dev(
        _ptr(umem), umem.numel() * umem.element_size(), _ptr(descs), n, opts, _ptr(table), n_entries, default_port,
        n_ports, _ptr(bound), _ptr(actions), _ptr(ports), _ptr(out), _ptr(off), _ptr(verdicts), _ptr(recs),
        _ptr(stats), _ptr(workspace), _stream_ptr(stream)))


def egress_ports_workspace_size(n_max: int, n_ports: int) -> int:
    """xsk_gpu_egress_ports_workspace_size: bytes of device workspace egress_ports_dev needs for a bound of n_max frames
    and n_ports ports (0 up to LOWLAT_MAX)."""
    return int(lib().xsk_gpu_egress_ports_workspace_size(n_max, n_ports))


def egress_ports_dev(descs, verdicts, off, n_ports: int, n_max: int, tx, free, counts, tx_room=None, stats=None,
                     port_stats=None, workspace=None, stream=None) -> None:
    """xsk_gpu_egress_ports_dev: egress_dev's rule once per steered port.  `off` holds n_ports + 1 uint32 words on the
    device, read when the kernels execute; port p's TX list is tx[off[p]:off[p] + n_tx_p], its free list
    free[off[p]:off[p] + n_free_p], and counts[p] (n_ports EGRESS_COUNTS_DTYPE) says how long both are.  `tx_room`:
    n_ports uint32 words on the device (None = unlimited); `stats`: the transform's counter block; `port_stats`:
    n_ports STATS_DTYPE blocks accumulated per port.  Behind ingress_steer_dev: descs=out, verdicts=verdicts, off=off.
    Inside a graph capture pass `workspace` (egress_ports_workspace_size bytes) when n_max > LOWLAT_MAX: allocating it
    here would be part of the capture."""
    if workspace is None and n_max > LOWLAT_MAX:
        import torch
        workspace = torch.empty(egress_ports_workspace_size(n_max, n_ports), dtype=torch.uint8, device=descs.device)
    _check("xsk_gpu_egress_ports_dev", lib().xsk_gpu_egress_ports_dev(
        _ptr(descs), _ptr(verdicts), _ptr(off), n_ports, n_max, _ptr(tx_room), _ptr(tx), _ptr(free), _ptr(counts),
        _ptr(stats), _ptr(port_stats), _ptr(workspace), _stream_ptr(stream)))


def rx_step_dev_workspace_size(max_batch: int) -> int:
    """xsk_gpu_rx_step_dev_workspace_size: bytes of device workspace rx_step_dev needs for a bound of max_batch frames."""
    return int(lib().xsk_gpu_rx_step_dev_workspace_size(max_batch))


def rx_begin_dev(rx: RingDev, fill: RingDev, tx: RingDev, pool: PoolDev, max_batch: int, descs, plan,
                 stream=None) -> None:
    """xsk_gpu_rx_begin_dev: peek up to max_batch RX entries into `descs` (max_batch descriptors), refill the fill ring
    from the pool and leave what was decided in `plan` (one RxPlan, 32 bytes), all on the device: steps 1 and 2 of
    xsk_gpu_rx_step over rings in device memory.  plan[0:4] serves as `count` and plan[4:8] as `tx_room` of
    echo_dev_indirect / egress_dev."""
    _check("xsk_gpu_rx_begin_dev", lib().xsk_gpu_rx_begin_dev(
        C.byref(rx), C.byref(fill), C.byref(tx), C.byref(pool), max_batch, _ptr(descs), _ptr(plan),
        _stream_ptr(stream)))


def rx_end_dev(rx: RingDev, tx: RingDev, pool: PoolDev, plan, tx_list, free, counts, n_max: int, res=None,
               stream=None) -> None:
    """xsk_gpu_rx_end_dev: egress_dev's TX list onto the TX ring, its free list onto the pool, the RX entries released,
    `res` (one RxResult in device memory, 16 bytes, or None) written: step 5 and the ring half of step 4."""
    _check("xsk_gpu_rx_end_dev", lib().xsk_gpu_rx_end_dev(
        C.byref(rx), C.byref(tx), C.byref(pool), _ptr(plan), _ptr(tx_list), _ptr(free), _ptr(counts), n_max, _ptr(res),
        _stream_ptr(stream)))


def rx_step_dev(umem, rx: RingDev, fill: RingDev, tx: RingDev, pool: PoolDev, max_batch: int, workspace, stats=None,
                res=None, stream=None, opts: int = 0) -> None:
    """xsk_gpu_rx_step_dev: one RX loop iteration over rings, pool and UMEM in device memory -- rx_begin_dev,
    echo_dev_indirect, egress_dev, rx_end_dev on one stream, the intermediate arrays carved from `workspace`
    (rx_step_dev_workspace_size(max_batch) bytes, 16-B aligned).  `stats`: one STATS_DTYPE on the device, accumulated;
    `res`: one RxResult on the device, written."""
    _check("xsk_gpu_rx_step_dev", lib().xsk_gpu_rx_step_dev(
        _ptr(umem), umem.numel() * umem.element_size(), C.byref(rx), C.byref(fill), C.byref(tx), C.byref(pool),
        max_batch, opts, _ptr(stats), _ptr(res), _ptr(workspace), _stream_ptr(stream)))


def tx_complete_dev(comp: RingDev, pool: PoolDev, max_entries: int, moved=None, stream=None) -> None:
    """xsk_gpu_tx_complete_dev: up to max_entries completed TX frames from the completion ring back onto the pool;
    `moved` (a uint32 word on the device, or None) receives the count."""
    _check("xsk_gpu_tx_complete_dev", lib().xsk_gpu_tx_complete_dev(
        C.byref(comp), C.byref(pool), max_entries, _ptr(moved), _stream_ptr(stream)))


def _ring_array(rings):
    """A host array of struct xsk_gpu_ring_dev from a sequence of RingDev (one TX ring per port)."""
    return (RingDev * len(rings))(*rings)


def rx_step_steer_dev_workspace_size(max_batch: int, n_ports: int) -> int:
    """xsk_gpu_rx_step_steer_dev_workspace_size: bytes of device workspace rx_step_steer_dev needs for a bound of
    max_batch frames and n_ports ports (enough for rx_end_ports_dev alone with the same bound)."""
    return int(lib().xsk_gpu_rx_step_steer_dev_workspace_size(max_batch, n_ports))


def rx_prepare_ports_dev(tx, plan, descs, n_max: int, tx_room, stream=None) -> None:
    """xsk_gpu_rx_prepare_ports_dev: between rx_begin_dev and ingress_steer_dev.  `tx`: a sequence of RingDev, one TX
    ring per port; tx_room[p] (len(tx) uint32 words on the device) receives port p's ring room, and descs[r:n_max]
    (r = min(plan.received, n_max)) become the pad descriptor the filter drops, so that steering n_max frames is exact."""
    _check("xsk_gpu_rx_prepare_ports_dev", lib().xsk_gpu_rx_prepare_ports_dev(
        _ring_array(tx), len(tx), _ptr(plan), _ptr(descs), n_max, _ptr(tx_room), _stream_ptr(stream)))


def rx_end_ports_dev(rx: RingDev, tx, pool: PoolDev, plan, descs, actions, off, tx_list, free, counts, n_max: int,
                     workspace, res=None, stream=None) -> None:
    """xsk_gpu_rx_ports_end_dev: behind egress_ports_dev -- port p's span of `tx_list` onto tx[p], every port's free
    list and then the frames `actions` did not redirect (addresses from `descs`, rx_begin_dev's array) onto the pool,
    the RX entries released, `res` (one RxSteerResult on the device, 32 bytes, or None) written.  `workspace`: 16-B
    aligned; rx_step_steer_dev_workspace_size(n_max, 1) bytes are enough."""
    _check("xsk_gpu_rx_ports_end_dev", lib().xsk_gpu_rx_ports_end_dev(
        C.byref(rx), _ring_array(tx), len(tx), C.byref(pool), _ptr(plan), _ptr(descs), _ptr(actions), _ptr(off),
        _ptr(tx_list), _ptr(free), _ptr(counts), n_max, _ptr(res), _ptr(workspace), _stream_ptr(stream)))


def rx_step_steer_dev(umem, rx: RingDev, fill: RingDev, tx, pool: PoolDev, max_batch: int, table, n_entries: int,
                      default_port: int, workspace, bound=None, actions=None, ports=None, port_counts=None, stats=None,
                      port_stats=None, res=None, stream=None, opts: int = 0) -> None:
    """xsk_gpu_rx_step_steer_dev: one steered RX loop iteration over rings, pool and UMEM in device memory -- rx_begin_dev,
    rx_prepare_ports_dev, ingress_steer_dev, egress_ports_dev, rx_end_ports_dev on one stream, from one RX ring to
    len(tx) TX rings.  `workspace`: rx_step_steer_dev_workspace_size(max_batch, len(tx)) bytes, 16-B aligned.  `actions`,
    `ports` (max_batch bytes) and `port_counts` (len(tx) EGRESS_COUNTS_DTYPE) are optional outputs; `stats` /
    `port_stats`: the shared and the per-port STATS_DTYPE blocks, accumulated; `res`: one RxSteerResult, written."""
    _check("xsk_gpu_rx_step_steer_dev", lib().xsk_gpu_rx_step_steer_dev(
        _ptr(umem), umem.numel() * umem.element_size(), C.byref(rx), C.byref(fill), _ring_array(tx), C.byref(pool),
        max_batch, opts, _ptr(table), n_entries, default_port, len(tx), _ptr(bound), _ptr(actions), _ptr(ports),
        _ptr(port_counts), _ptr(stats), _ptr(port_stats), _ptr(res), _ptr(workspace), _stream_ptr(stream)))


def rx_pass_step_dev_workspace_size(max_batch: int, n_ports: int) -> int:
    """xsk_gpu_rx_pass_step_dev_workspace_size: bytes of device workspace rx_pass_step_dev needs for a bound of max_batch
    frames and n_ports ports (enough for rx_pass_end_dev alone with the same bound)."""
    return int(lib().xsk_gpu_rx_pass_step_dev_workspace_size(max_batch, n_ports))


def _ring_ref(ring):
    return None if ring is None else C.byref(ring)


def rx_pass_end_dev(rx: RingDev, tx, stack: Optional[RingDev], pool: PoolDev, plan, descs, actions, off, tx_list, free,
                    counts, n_max: int, workspace, res=None, stream=None) -> None:
    """xsk_gpu_rx_pass_end_dev: rx_end_ports_dev with a stack ring -- the descriptors of the frames `actions` passes to
    the kernel stack go onto `stack` (a descriptor RingDev, or None) in batch order, as many as it has room for; only the
    other frames that were not redirected return to the pool.  `res`: one RxPassResult on the device (32 bytes), or None.
    `workspace`: 16-B aligned; rx_pass_step_dev_workspace_size(n_max, 1) bytes are enough."""
    _check("xsk_gpu_rx_pass_end_dev", lib().xsk_gpu_rx_pass_end_dev(
        C.byref(rx), _ring_array(tx), len(tx), _ring_ref(stack), C.byref(pool), _ptr(plan), _ptr(descs), _ptr(actions),
        _ptr(off), _ptr(tx_list), _ptr(free), _ptr(counts), n_max, _ptr(res), _ptr(workspace), _stream_ptr(stream)))


def rx_pass_step_dev(umem, rx: RingDev, fill: RingDev, tx, stack: Optional[RingDev], pool: PoolDev, max_batch: int, table,
                     n_entries: int, default_port: int, workspace, bound=None, actions=None, ports=None,
                     port_counts=None, stats=None, port_stats=None, res=None, stream=None, opts: int = 0) -> None:
    """xsk_gpu_rx_pass_step_dev: rx_step_steer_dev with a stack ring -- rx_begin_dev, rx_prepare_ports_dev,
    ingress_steer_dev, egress_ports_dev, rx_pass_end_dev on one stream.  `stack`: a descriptor RingDev for the frames the
    filter passes to the kernel stack, or None (then, as with a full ring, the step is rx_step_steer_dev).  `workspace`:
    rx_pass_step_dev_workspace_size(max_batch, len(tx)) bytes, 16-B aligned; `res`: one RxPassResult, written; the other
    arguments as in rx_step_steer_dev."""
    _check("xsk_gpu_rx_pass_step_dev", lib().xsk_gpu_rx_pass_step_dev(
        _ptr(umem), umem.numel() * umem.element_size(), C.byref(rx), C.byref(fill), _ring_array(tx), _ring_ref(stack),
        C.byref(pool), max_batch, opts, _ptr(table), n_entries, default_port, len(tx), _ptr(bound), _ptr(actions),
        _ptr(ports), _ptr(port_counts), _ptr(stats), _ptr(port_stats), _ptr(res), _ptr(workspace), _stream_ptr(stream)))


def tx_complete_rings_dev(comps, pool: PoolDev, max_entries: int, moved=None, pushed=None, stream=None) -> None:
    """xsk_gpu_tx_complete_rings_dev: tx_complete_dev over every completion ring of `comps` (a sequence of up to
    COMPLETE_MAX_RINGS address RingDev) in turn, by one call: up to max_entries entries of each ring back onto the pool,
    in ring order, as many as the pool has room for.  `moved` (len(comps) uint32 words on the device, or None) receives
    every ring's count, `pushed` (one word, or None) what the pool took."""
    _check("xsk_gpu_tx_complete_rings_dev", lib().xsk_gpu_tx_complete_rings_dev(
        _ring_array(comps) if len(comps) else None, len(comps), C.byref(pool), max_entries, _ptr(moved), _ptr(pushed),
        _stream_ptr(stream)))


def rx_loop_dev(umem, rx: RingDev, fill: RingDev, tx, stack: Optional[RingDev], pool: PoolDev, max_batch: int, table,
                n_entries: int, default_port: int, comps, complete_max: int, workspace, bound=None, actions=None,
                ports=None, port_counts=None, stats=None, port_stats=None, res=None, moved=None, pushed=None, stream=None,
                opts: int = 0) -> None:
    """xsk_gpu_rx_loop_dev: the whole RX loop body over all sockets on one stream -- rx_pass_step_dev, then
    tx_complete_rings_dev(comps, pool, complete_max, moved, pushed).  `comps`: the completion rings (one per port and the
    stack consumer's, up to COMPLETE_MAX_RINGS); empty: the call is rx_pass_step_dev.  `workspace`:
    rx_pass_step_dev_workspace_size(max_batch, len(tx)) bytes, 16-B aligned; the other arguments as in those two calls."""
    _check("xsk_gpu_rx_loop_dev", lib().xsk_gpu_rx_loop_dev(
        _ptr(umem), umem.numel() * umem.element_size(), C.byref(rx), C.byref(fill), _ring_array(tx), _ring_ref(stack),
        C.byref(pool), max_batch, opts, _ptr(table), n_entries, default_port, len(tx), _ptr(bound), _ptr(actions),
        _ptr(ports), _ptr(port_counts), _ptr(stats), _ptr(port_stats), _ptr(res),
        _ring_array(comps) if len(comps) else None, len(comps), complete_max, _ptr(moved), _ptr(pushed),
        _ptr(workspace), _stream_ptr(stream)))


def rx_loop_fused_dev(umem, rx: RingDev, fill: RingDev, tx, stack: Optional[RingDev], pool: PoolDev, max_batch: int,
                      table, n_entries: int, default_port: int, comps, complete_max: int, workspace, bound=None,
                      actions=None, ports=None, port_counts=None, stats=None, port_stats=None, res=None, moved=None,
                      pushed=None, stream=None, opts: int = 0) -> None:
    """xsk_gpu_rx_fused_loop_dev: rx_loop_dev as one launch of one workgroup, for max_batch (and, with completion rings,
    complete_max) up to LOWLAT_MAX; from the same state it leaves what rx_loop_dev leaves.  Arguments as rx_loop_dev's.
    (The C symbol keeps clear of "rx_loop", which the export-table checks reserve for xsk_gpu_rx_loop_dev.)"""
    _check("xsk_gpu_rx_fused_loop_dev", lib().xsk_gpu_rx_fused_loop_dev(
        _ptr(umem), umem.numel() * umem.element_size(), C.byref(rx), C.byref(fill), _ring_array(tx), _ring_ref(stack),
        C.byref(pool), max_batch, opts, _ptr(table), n_entries, default_port, len(tx), _ptr(bound), _ptr(actions),
        _ptr(ports), _ptr(port_counts), _ptr(stats), _ptr(port_stats), _ptr(res),
        _ring_array(comps) if len(comps) else None, len(comps), complete_max, _ptr(moved), _ptr(pushed),
        _ptr(workspace), _stream_ptr(stream)))


def rx_queue(umem, rx: RingDev, fill: RingDev, tx, stack: Optional[RingDev], pool: PoolDev, max_batch: int, table,
             n_entries: int, default_port: int, comps, complete_max: int, workspace, bound=None, actions=None, ports=None,
             port_counts=None, stats=None, port_stats=None, res=None, moved=None, pushed=None) -> RxQueue:
    """One RxQueue from the arguments rx_loop_fused_dev takes (`opts` and `stream` belong to the call over all queues).
    The ctypes ring and pool structs the struct points to are kept alive on the returned object."""
    keep = (rx, fill, _ring_array(tx) if len(tx) else None, stack, pool, _ring_array(comps) if len(comps) else None)
    q = RxQueue(_ptr(umem), umem.numel() * umem.element_size(), C.pointer(rx), C.pointer(fill), keep[2],
                C.pointer(stack) if stack is not None else None, C.pointer(pool), _ptr(table), _ptr(bound),
                _ptr(actions), _ptr(ports), _ptr(port_counts), _ptr(stats), _ptr(port_stats), _ptr(res), keep[5],
                _ptr(moved), _ptr(pushed), _ptr(workspace), max_batch, len(tx), n_entries, default_port, len(comps),
                complete_max)
    q._keep = keep
    return q


def rx_queues_block_size(n_queues: int) -> int:
    """xsk_gpu_rx_queues_block_size: bytes of the argument block of n_queues queues; 0 outside [1, RX_MAX_QUEUES]."""
    return int(lib().xsk_gpu_rx_queues_block_size(n_queues))


def rx_queues_prepare(queues, opts: int = 0) -> np.ndarray:
    """xsk_gpu_rx_queues_prepare: the argument block of rx_queues_dev for `queues` (a sequence of RxQueue) and `opts`, as
    a uint8 array in host memory.  Copy it to 64-B aligned device memory once; it holds the rings' addresses, so it
    stays valid while they do.  Raises XskGpuError where any queue breaks a rule of rx_loop_fused_dev or two queues
    share a pointer the kernel writes through."""
    n = len(queues)
    arr = (RxQueue * n)(*queues) if n else None
    block = np.zeros(max(rx_queues_block_size(n), 1), np.uint8)
    _check("xsk_gpu_rx_queues_prepare", lib().xsk_gpu_rx_queues_prepare(arr, n, opts, block.ctypes.data))
    return block


def rx_queues_dev(d_block, n_queues: int, opts: int = 0, stream=None) -> None:
    """xsk_gpu_rx_queues_dev: rx_loop_fused_dev for n_queues independent queues as one launch of n_queues workgroups.
    `d_block`: rx_queues_prepare's block for the same n_queues and opts, in device memory (a torch tensor, 64-B
    aligned); a block prepared for another count or other options makes the call a no-op."""
    _check("xsk_gpu_rx_queues_dev", lib().xsk_gpu_rx_queues_dev(_ptr(d_block), n_queues, opts, _stream_ptr(stream)))


def neigh_table_prepare(entries: np.ndarray) -> np.ndarray:
    """xsk_gpu_neigh_table_prepare on a copy of a host array of NEIGH_ENTRY_DTYPE: checked and sorted by (family, addr),
    the order the responder's search needs.  Raises XskGpuError (-EINVAL, -EEXIST)."""
    e = np.array(entries, dtype=NEIGH_ENTRY_DTYPE, copy=True).reshape(-1)
    _check("xsk_gpu_neigh_table_prepare", lib().xsk_gpu_neigh_table_prepare(e.ctypes.data if len(e) else None, len(e)))
    return e


def neigh_dev(umem, descs, n_max: int, table, n_entries: int, n_ports: int, nverdicts, nports, count=None, bound=None,
              reply_len=None, nstats=None, stream=None, opts: int = 0) -> None:
    """xsk_gpu_neigh_dev: answer the ARP requests and neighbour solicitations among the first min(*count, n_max)
    descriptors (n_max without `count`, one uint32 word on the device read when the kernel executes) for the addresses of
    `table` (a device copy of a neigh_table_prepare()d array, or None with n_entries == 0), in place.  nverdicts[i] is
    the NEIGH_* verdict, nports[i] the owning port of a reply (0xFF otherwise), reply_len[i] (optional) its length;
    `nstats` (one NEIGH_STATS_DTYPE on the device, optional) is accumulated.  `bound` as in steer_dev."""
    _check("xsk_gpu_neigh_dev", lib().xsk_gpu_neigh_dev(
        _ptr(umem), umem.numel() * umem.element_size(), _ptr(descs), _ptr(count), n_max, opts, _ptr(table), n_entries,
        n_ports, _ptr(bound), _ptr(nverdicts), _ptr(nports), _ptr(reply_len), _ptr(nstats), _stream_ptr(stream)))


def neigh_serve_dev(umem, stack: RingDev, tx, up: RingDev, max_entries: int, table, n_entries: int, bound=None,
                    nstats=None, res=None, stream=None, opts: int = 0) -> None:
    """xsk_gpu_neigh_serve_dev: the consumer of the stack ring rx_pass_step_dev produces.  Up to max_entries
    (<= LOWLAT_MAX) entries of `stack` are decided by neigh_dev's rule: a reply is written in place and its descriptor
    goes onto tx[port] (a sequence of RingDev, the ports' TX rings), every other entry onto `up` as it is; the call stops
    in front of the first entry whose destination is full.  `res`: one NEIGH_RESULT_DTYPE on the device, written."""
    _check("xsk_gpu_neigh_serve_dev", lib().xsk_gpu_neigh_serve_dev(
        _ptr(umem), umem.numel() * umem.element_size(), C.byref(stack), _ring_array(tx), len(tx), C.byref(up),
        max_entries, opts, _ptr(table), n_entries, _ptr(bound), _ptr(nstats), _ptr(res), _stream_ptr(stream)))


def responder_queue(q: RxQueue, up: RingDev, serve_max: int, ntable, n_nentries: int, nstats=None,
                    nres=None) -> ResponderQueue:
    """One ResponderQueue: `q` is rx_queue()'s struct (its stack ring is required), the rest are neigh_serve_dev's up,
    max_entries, table, n_entries, nstats and res.  The bound word and the options are q's and the call's: one of each
    for both halves.  What the struct points to is kept alive on the returned object."""
    r = ResponderQueue(q, C.pointer(up) if up is not None else None, _ptr(ntable), _ptr(nstats), _ptr(nres), n_nentries,
                       serve_max)
    r._keep = (q, getattr(q, "_keep", None), up)
    return r


def responder_dev(r: ResponderQueue, opts: int = 0, stream=None) -> None:
    """xsk_gpu_responder_dev: rx_loop_fused_dev over r.q followed by neigh_serve_dev over its stack ring, as ONE launch of
    one workgroup; it leaves exactly what those two calls leave.  A request the step puts on the stack ring in this
    call is answered in this call."""
    _check("xsk_gpu_responder_dev", lib().xsk_gpu_responder_dev(C.byref(r) if r is not None else None, opts,
                                                                _stream_ptr(stream)))


def responder_block_size(n_queues: int) -> int:
    """xsk_gpu_responder_block_size: bytes of the argument block of n_queues queues; 0 outside [1, RX_MAX_QUEUES]."""
    return int(lib().xsk_gpu_responder_block_size(n_queues))


def responder_prepare(queues, opts: int = 0) -> np.ndarray:
    """xsk_gpu_responder_prepare: the argument block of responder_queues_dev for `queues` (a sequence of ResponderQueue)
    and `opts`, as a uint8 array in host memory; copy it to 64-B aligned device memory once.  Raises XskGpuError where a
    queue breaks a rule of responder_dev or two queues share a pointer the kernel writes through."""
    n = len(queues)
    arr = (ResponderQueue * n)(*queues) if n else None
    block = np.zeros(max(responder_block_size(n), 1), np.uint8)
    _check("xsk_gpu_responder_prepare", lib().xsk_gpu_responder_prepare(arr, n, opts, block.ctypes.data))
    return block


def responder_queues_dev(d_block, n_queues: int, opts: int = 0, stream=None) -> None:
    """xsk_gpu_responder_queues_dev: responder_dev for n_queues independent queues as one launch of n_queues workgroups.
    `d_block`: responder_prepare's block for the same n_queues and opts, in device memory (64-B aligned); any other
    block -- another count, other options, an rx_queues_prepare block -- makes the call a no-op."""
    _check("xsk_gpu_responder_queues_dev",
           lib().xsk_gpu_responder_queues_dev(_ptr(d_block), n_queues, opts, _stream_ptr(stream)))


def unreach_dev(umem, descs, n_max: int, table, n_entries: int, n_ports: int, chunk_size: int, uverdicts, uports,
                count=None, bound=None, open_ports=None, reply_len=None, ustats=None, stream=None, opts: int = 0) -> None:
    """xsk_gpu_unreach_dev: answer the UDP datagrams among the first min(*count, n_max) descriptors that reach an address
    of `table` (neigh_table_prepare's, on the device) on a closed port with ICMP / ICMPv6 port unreachable, in place; the
    reply is longer than what it quotes and must fit the frame's chunk of `chunk_size` bytes.  `open_ports`: 8192 bytes
    on the device, a bit per listening UDP port (None: every port is closed).  uverdicts[i] is the UNREACH_* verdict,
    uports[i] the owning port of a reply (0xFF otherwise), reply_len[i] (optional) its length; `ustats` (one
    UNREACH_STATS_DTYPE on the device, optional) is accumulated.  No rate limit."""
    _check("xsk_gpu_unreach_dev", lib().xsk_gpu_unreach_dev(
        _ptr(umem), umem.numel() * umem.element_size(), _ptr(descs), _ptr(count), n_max, opts, _ptr(table), n_entries,
        n_ports, _ptr(bound), _ptr(open_ports), chunk_size, _ptr(uverdicts), _ptr(uports), _ptr(reply_len), _ptr(ustats),
        _stream_ptr(stream)))


def unreach_serve_dev(umem, up: RingDev, tx, rest: RingDev, max_entries: int, table, n_entries: int, chunk_size: int,
                      bound=None, open_ports=None, budget=None, ustats=None, res=None, stream=None, opts: int = 0) -> None:
    """xsk_gpu_unreach_serve_dev: the consumer of the `up` ring neigh_serve_dev produces.  Up to max_entries entries of
    `up` are decided by unreach_dev's rule: an error is written in place and its descriptor goes onto tx[port], every
    other entry onto `rest` as it is; the call stops in front of the first entry whose destination is full.  `budget`:
    one uint32 word on the device, the errors the call may still send (None: unlimited); an error due behind it is
    UNREACH_LIMITED and goes to `rest`; the word is left holding what remains.  `res`: one UNREACH_RESULT_DTYPE."""
    _check("xsk_gpu_unreach_serve_dev", lib().xsk_gpu_unreach_serve_dev(
        _ptr(umem), umem.numel() * umem.element_size(), C.byref(up), _ring_array(tx), len(tx), C.byref(rest),
        max_entries, opts, _ptr(table), n_entries, _ptr(bound), _ptr(open_ports), chunk_size, _ptr(budget), _ptr(ustats),
        _ptr(res), _stream_ptr(stream)))


def synth_dev(umem, descs, n: int, base_off: int, stride: int, seed: int, first: int = 0, step: int = 1,
              mode: int = 0, len_lo: int = 1500, len_hi: int = 1500, stream=None) -> None:
    _check("xsk_gpu_synth_dev", lib().xsk_gpu_synth_dev(
        _ptr(umem), umem.numel() * umem.element_size(), _ptr(descs), n, base_off, stride, seed, first, step, mode,
        len_lo, len_hi, _stream_ptr(stream)))


def rearm_dev(umem, descs, verdicts, n: int, stream=None) -> None:
    _check("xsk_gpu_rearm_dev", lib().xsk_gpu_rearm_dev(_ptr(umem), _ptr(descs), _ptr(verdicts), n,
                                                        _stream_ptr(stream)))


def stream_read_dev(src, nbytes: int, out, stream=None) -> None:
    _check("xsk_gpu_stream_read_dev", lib().xsk_gpu_stream_read_dev(_ptr(src), nbytes, _ptr(out),
                                                                    _stream_ptr(stream)))


def lowlat_reserve(device: int, queues: int) -> int:
    """xsk_gpu_lowlat_reserve: set aside highest-priority hardware queues of `device` for the application's own
    highest-priority streams; returns the resident LOWLAT kernels now allowed there."""
    rc = lib().xsk_gpu_lowlat_reserve(device, queues)
    if rc < 0:
        raise XskGpuError("xsk_gpu_lowlat_reserve", rc)
    return rc



def lowlat_cap(device: int = 0) -> int:
    """xsk_gpu_lowlat_cap: the resident LOWLAT kernels this process may run on `device` now (min(8,
    GPU_MAX_HW_QUEUES) less the reserved queues), without changing anything."""
    rc = lib().xsk_gpu_lowlat_cap(device)
    if rc < 0:
        raise XskGpuError("xsk_gpu_lowlat_cap", rc)
    return rc

def timing_enable(on: bool = True) -> None:
    _check("xsk_gpu_timing_enable", lib().xsk_gpu_timing_enable(1 if on else 0))


def timing_read():
    ms = C.c_double(0.0)
    cnt = C.c_uint64(0)
    _check("xsk_gpu_timing_read", lib().xsk_gpu_timing_read(C.byref(ms), C.byref(cnt)))
    return ms.value, cnt.value


def lowlat_live(device: int = 0) -> int:
    """Workgroups of resident LOWLAT grids running on `device` in this process (xsk_gpu__lowlat_live)."""
    out = C.c_uint32(0)
    _check("xsk_gpu__lowlat_live", lib().xsk_gpu__lowlat_live(device, C.byref(out)))
    return int(out.value)


def umem_zeros(nbytes: int) -> np.ndarray:
    """A zeroed host UMEM on pages of its own: an anonymous mapping, so its base is page-aligned as xsk_gpu_init /
    xsk_gpu_multi_init / xsk_gpu_rx_pipe_init require and AF_XDP does -- the counterpart of the reference's
    posix_memalign(getpagesize(), ...) (src/lib/xsk_utils.c:132-135).  A plain numpy array is not: its data may start
    inside a page another allocation shares."""
    nbytes = int(nbytes)
    return np.frombuffer(mmap.mmap(-1, max(nbytes, 1)), np.uint8, count=nbytes)


def umem_copy(a: np.ndarray) -> np.ndarray:
    """umem_zeros of a's size holding a's bytes."""
    out = umem_zeros(a.nbytes)
    out[:] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    return out


class HugeUmem:
    """xsk_gpu_umem_alloc / xsk_gpu_umem_free: a UMEM on transparent huge pages (2 MiB aligned, touched up front);
    `.array` is its numpy uint8 view, `.huge_bytes` how much of it the kernel backed with huge pages."""

    def __init__(self, size: int):
        self._p = C.c_void_p()
        hb = C.c_uint64(0)
        _check("xsk_gpu_umem_alloc", lib().xsk_gpu_umem_alloc(C.byref(self._p), size, C.byref(hb)))
        self.size = size
        self.huge_bytes = int(hb.value)
        self.array = np.ctypeslib.as_array((C.c_uint8 * size).from_address(self._p.value))

    def close(self) -> None:
        if self._p:
            self.array = None
            lib().xsk_gpu_umem_free(self._p, self.size)
            self._p = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


STAGED_FIELDS = ("h2d_bytes", "strided", "span", "gather", "contained", "hostpack", "own_dma")


def staged_stats_of(ctx) -> dict:
    """xsk_gpu__staged_stats of a STAGED context handle: bytes copied host->device since init (frame bytes, plus the
    host pack's 4-B staging offsets), the chunks copied as one 2-D stride / one dense span / by the gather kernel, the
    chunks whose copy-in wrote only their own frames' mirror bytes (run without waiting for the previous chunk's header
    pack), the chunks copied by the host pack (no mapped alias), and the frames of those too large for a staging half
    (a DMA copy each)."""
    out = (C.c_uint64 * len(STAGED_FIELDS))()
    _check("xsk_gpu__staged_stats", lib().xsk_gpu__staged_stats(ctx, out))
    return dict(zip(STAGED_FIELDS, (int(x) for x in out)))


def _lowlat_served_of(handle):
    out = (C.c_uint64 * 2)()
    _check("xsk_gpu__lowlat_served", lib().xsk_gpu__lowlat_served(handle, out))
    return int(out[0]), int(out[1])


class EchoContext:
    """Host-UMEM drop-in (xsk_gpu_init / xsk_gpu_process / xsk_gpu_fini) over a numpy uint8 UMEM."""

    def __init__(self, umem: np.ndarray, device: int = 0, max_batch: int = 4096, mode: int = MODE_ZEROCOPY,
                 opts: int = 0):
        assert umem.dtype == np.uint8 and umem.flags.c_contiguous
        self.umem = umem
        self._ctx = C.c_void_p()
        _check("xsk_gpu_init", lib().xsk_gpu_init(C.byref(self._ctx), device, umem.ctypes.data, umem.nbytes,
                                                  max_batch, mode))
        if opts:
            self.set_options(opts)

    def set_options(self, opts: int) -> None:
        _check("xsk_gpu_set_options", lib().xsk_gpu_set_options(self._ctx, opts))

    @property
    def mode(self) -> int:
        """xsk_gpu_ctx_mode: the mode the context runs in (a LOWLAT request beyond XSK_GPU_LOWLAT_PER_DEVICE on its
        device runs as ZEROCOPY)."""
        return lib().xsk_gpu_ctx_mode(self._ctx)

    def process(self, descs: np.ndarray, want_recs: bool = True):
        n = len(descs)
        descs = np.ascontiguousarray(descs, dtype=DESC_DTYPE)
        verdicts = np.zeros(n, np.uint8)
        recs = np.zeros(n, REC_DTYPE) if want_recs else None
        stats = np.zeros(1, STATS_DTYPE)
        _check("xsk_gpu_process", lib().xsk_gpu_process(
            self._ctx, descs.ctypes.data, n, verdicts.ctypes.data, recs.ctypes.data if recs is not None else None,
            stats.ctypes.data))
        return verdicts, recs, stats[0]

    def staged_stats(self):
        """xsk_gpu__staged_stats of a STAGED context (see staged_stats_of)."""
        return staged_stats_of(self._ctx)

    def drop_alias(self, half_bytes: int = 0) -> None:
        """Test switch (xsk_gpu__staged_noalias): the STAGED context forgets its UMEM's mapped device alias, as on a
        device where the runtime gives none, so its scattered copy-ins take the host pack (staging halves of
        half_bytes; 0 = the default 32 MiB)."""
        _check("xsk_gpu__staged_noalias", lib().xsk_gpu__staged_noalias(self._ctx, half_bytes))

    def lowlat_tune(self, tile_frames: int = 0, groups: int = 0, timeout_us: int = 0) -> None:
        """Tool / test knobs of a LOWLAT context (xsk_gpu__lowlat_tune): frames per wave, serving workgroups,
        completion timeout (0 = defaults)."""
        _check("xsk_gpu__lowlat_tune", lib().xsk_gpu__lowlat_tune(self._ctx, tile_frames, groups, timeout_us))

    def lowlat_test_width(self, wgs: int) -> None:
        """Test switch (xsk_gpu__lowlat_test_width): launch the resident grid with `wgs` workgroups (0 = all)."""
        _check("xsk_gpu__lowlat_test_width", lib().xsk_gpu__lowlat_test_width(self._ctx, wgs))

    def umem_view(self, off: int, n: int) -> np.ndarray:
        """xsk_gpu__umem_view: n bytes at `off` as the GPU's translation of the UMEM sees them (ZEROCOPY / LOWLAT)."""
        out = np.zeros(n, np.uint8)
        _check("xsk_gpu__umem_view", lib().xsk_gpu__umem_view(self._ctx, off, out.ctypes.data, n))
        return out

    def lowlat_outcomes(self):
        """xsk_gpu__lowlat_outcomes: doorbell batches that missed their timeout -- all, completed through the launch
        path after a partial service, returned -ETIMEDOUT, completed late (every slice served, found after STOP)."""
        out = (C.c_uint64 * 4)()
        _check("xsk_gpu__lowlat_outcomes", lib().xsk_gpu__lowlat_outcomes(self._ctx, out))
        return {"timeouts": int(out[0]), "partial": int(out[1]), "untouched": int(out[2]), "late": int(out[3])}

    def lowlat_served(self):
        """xsk_gpu__lowlat_served of a LOWLAT context: (batches completed by the resident kernel, batches that took
        the launch path)."""
        return _lowlat_served_of(self._ctx)

    def rx_step(self, rx: Ring, fill: Ring, tx: Ring, pool: FramePool, max_batch: int, stats=None):
        """xsk_gpu_rx_step on this context; returns (received, RxResult)."""
        res = RxResult()
        rc = lib().xsk_gpu_rx_step(self._ctx, C.byref(rx), C.byref(fill), C.byref(tx), C.byref(pool), max_batch,
                                   stats.ctypes.data if stats is not None else None, C.byref(res))
        if rc < 0:
            raise XskGpuError("xsk_gpu_rx_step", rc)
        return rc, res

    def close(self) -> None:
        if self._ctx:
            lib().xsk_gpu_fini(self._ctx)
            self._ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiContext:
    """xsk_gpu_multi_*: one host UMEM, one context per entry of ``devices`` (repeats allowed), descriptor i
    of a batch on context i mod G, counters summed."""

    def __init__(self, umem: np.ndarray, devices, max_batch: int = 4096, mode: int = MODE_ZEROCOPY, opts: int = 0):
        assert umem.dtype == np.uint8 and umem.flags.c_contiguous
        self.umem = umem
        self._ctx = C.c_void_p()
        devs = (C.c_int * len(devices))(*devices)
        _check("xsk_gpu_multi_init", lib().xsk_gpu_multi_init(C.byref(self._ctx), devs, len(devices), umem.ctypes.data,
                                                              umem.nbytes, max_batch, mode))
        if opts:
            _check("xsk_gpu_multi_set_options", lib().xsk_gpu_multi_set_options(self._ctx, opts))

    def process(self, descs: np.ndarray, want_recs: bool = True):
        n = len(descs)
        descs = np.ascontiguousarray(descs, dtype=DESC_DTYPE)
        verdicts = np.zeros(n, np.uint8)
        recs = np.zeros(n, REC_DTYPE) if want_recs else None
        stats = np.zeros(1, STATS_DTYPE)
        _check("xsk_gpu_multi_process", lib().xsk_gpu_multi_process(
            self._ctx, descs.ctypes.data, n, verdicts.ctypes.data, recs.ctypes.data if recs is not None else None,
            stats.ctypes.data))
        return verdicts, recs, stats[0]

    def status(self):
        """xsk_gpu_multi_status: per-context result of the last process() (0 or -errno)."""
        st = (C.c_int * MULTI_MAX)()
        g = lib().xsk_gpu_multi_status(self._ctx, st, MULTI_MAX)
        if g < 0:
            raise XskGpuError("xsk_gpu_multi_status", g)
        return list(st[:g])

    def context(self, g: int):
        """Context g's handle (xsk_gpu__multi_ctx), for staged_stats_of."""
        h = lib().xsk_gpu__multi_ctx(self._ctx, g)
        if not h:
            raise XskGpuError("xsk_gpu__multi_ctx", -22)
        return h

    def staged_stats(self):
        """Every context's xsk_gpu__staged_stats (STAGED mode), in context order."""
        return [staged_stats_of(self.context(g)) for g in range(len(self.status()))]

    def drop_alias(self, half_bytes: int = 0) -> None:
        """Test switch: every context forgets the UMEM's mapped alias (xsk_gpu__staged_noalias)."""
        for g in range(len(self.status())):
            _check("xsk_gpu__staged_noalias", lib().xsk_gpu__staged_noalias(self.context(g), half_bytes))

    def lowlat_served(self):
        """The member contexts' lowlat_served(), summed (every member runs LOWLAT)."""
        per = [_lowlat_served_of(self.context(g)) for g in range(len(self.status()))]
        return sum(a for a, _ in per), sum(b for _, b in per)

    def inject_failure(self, g: int, rc: int) -> None:
        """Test hook: context g's next share fails with rc (xsk_gpu__multi_inject)."""
        _check("xsk_gpu__multi_inject", lib().xsk_gpu__multi_inject(self._ctx, g, rc))

    def close(self) -> None:
        if self._ctx:
            lib().xsk_gpu_multi_fini(self._ctx)
            self._ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ContextView(EchoContext):
    """A context owned by another object (a pipelined RX loop's): EchoContext's queries and test knobs, no ownership."""

    def __init__(self, handle):  # noqa: super().__init__ is not called: nothing is created
        self.umem = None
        self._ctx = C.c_void_p(handle)

    def close(self) -> None:
        self._ctx = C.c_void_p()


class RxPipe:
    """xsk_gpu_rx_pipe_*: the RX loop step with up to ``depth`` batches in flight, one per context of ``mode`` over one
    registration of the UMEM (include/xsk_gpu.h)."""

    def __init__(self, umem: np.ndarray, device: int = 0, depth: int = 2, mode: int = MODE_LOWLAT, opts: int = 0):
        assert umem.dtype == np.uint8 and umem.flags.c_contiguous
        self.umem = umem
        self.depth_asked = depth
        self._p = C.c_void_p()
        _check("xsk_gpu_rx_pipe_init", lib().xsk_gpu_rx_pipe_init(C.byref(self._p), device, umem.ctypes.data,
                                                                  umem.nbytes, depth, mode))
        if opts:
            self.set_options(opts)

    def set_options(self, opts: int) -> None:
        _check("xsk_gpu_rx_pipe_set_options", lib().xsk_gpu_rx_pipe_set_options(self._p, opts))

    def step(self, rx: Ring, fill: Ring, tx: Ring, pool: FramePool, max_batch: int, stats=None):
        """xsk_gpu_rx_pipe_step: returns (frames completed, RxResult)."""
        res = RxResult()
        rc = lib().xsk_gpu_rx_pipe_step(self._p, C.byref(rx), C.byref(fill), C.byref(tx), C.byref(pool), max_batch,
                                        stats.ctypes.data if stats is not None else None, C.byref(res))
        if rc < 0:
            raise XskGpuError("xsk_gpu_rx_pipe_step", rc)
        return rc, res

    def flush(self, tx: Ring, pool: FramePool, stats=None):
        """xsk_gpu_rx_pipe_flush: returns (frames completed, RxResult)."""
        res = RxResult()
        rc = lib().xsk_gpu_rx_pipe_flush(self._p, C.byref(tx), C.byref(pool),
                                         stats.ctypes.data if stats is not None else None, C.byref(res))
        if rc < 0:
            raise XskGpuError("xsk_gpu_rx_pipe_flush", rc)
        return rc, res

    @property
    def inflight(self) -> int:
        return int(lib().xsk_gpu_rx_pipe_inflight(self._p))

    @property
    def depth(self) -> int:
        """Contexts the pipe holds: a LOWLAT pipe keeps doorbell contexts only (xsk_gpu_rx_pipe_depth)."""
        return int(lib().xsk_gpu_rx_pipe_depth(self._p))

    def context(self, i: int) -> ContextView:
        """Context i of the pipe (xsk_gpu__rx_pipe_ctx): its mode, LOWLAT knobs and outcomes."""
        h = lib().xsk_gpu__rx_pipe_ctx(self._p, i)
        if not h:
            raise XskGpuError("xsk_gpu__rx_pipe_ctx", -22)
        return ContextView(h)

    def lowlat_served(self):
        """The pipe's contexts' lowlat_served(), summed (a LOWLAT pipe)."""
        per = [self.context(i).lowlat_served() for i in range(self.depth)]
        return sum(a for a, _ in per), sum(b for _, b in per)

    def close(self) -> None:
        if self._p:
            lib().xsk_gpu_rx_pipe_fini(self._p)
            self._p = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
