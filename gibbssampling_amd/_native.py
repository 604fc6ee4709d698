"""ctypes binding of libgibbs_hip.so (include/gibbs_hip.h).

The product path is the HIP library only: if the shared object is missing or
cannot be loaded this module raises -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
REPO_DIR = PKG_DIR.parent
LIB_PATH = PKG_DIR / "libgibbs_hip.so"
HEADER_PATH = REPO_DIR / "include" / "gibbs_hip.h"

GS_OK = 0
GS_E_ARG = 1
GS_E_ROULETTE_OVERRUN = 2
GS_E_OVERFLOW = 3
GS_E_HIP = 4
GS_E_RCCL = 5
GS_E_STATE = 6
GS_E_UNSUPPORTED = 7
UNIQUE_ID_BYTES = 128
SCAN_CERTIFIED = 0
SCAN_EXACT = 1
IPC_HANDLE_BYTES = 64  # include/gibbs_hip.h GS_IPC_HANDLE_BYTES
LOG2_ERR_BUDGET = 2.0 ** -22  # gs_common.h kLog2AbsErr
EXP2_ERR_BUDGET = 2.0 ** -22  # gs_common.h kExp2RelErr
STAT_NAMES = ("exact_rescans", "serial_picks", "rescan_flagged", "rescan_recheck",
              "rescan_total", "rescan_no_lane", "rescan_boundary", "rescan_between_lanes",
              "bg_path", "bg_picks", "live_band", "live_list_full", "live_no_motif",
              "desc_oob")


# Spellings of the tuning fields in the tools' A/B specs (NAME=value)
TUNING_ALIASES = {
    "GS_BLOCKS_PER_CU": "blocks_per_cu_cap", "GS_GROUP_LANES": "group_lanes",
    "GS_SWEEP_WAVES": "sweep_waves", "GS_DNA": "dna_mode", "GS_DNA_G": "dna_G",
    "GS_GRAPH": "graph_mode", "GS_SITE_COOP": "site_coop", "GS_COOP_RATE": "coop_rate",
    "GS_GREEDY_COOP": "motif_coop", "GS_SITE_DT16": "site_dt16",
    "GS_SITE_EXIT_CHUNK": "site_exit_chunk", "GS_SITE_EXIT_RATIO": "site_exit_ratio",
    "GS_GREEDY_EXIT_CHUNK": "greedy_exit_chunk", "GS_GREEDY_EXIT_RATIO": "greedy_exit_ratio",
    "GS_GREEDY_WAVES": "greedy_waves", "GS_MULTI_GREEDY_THREADS": "multi_greedy_threads",
    "GS_MULTI_SPEC_SLOTS": "multi_spec_slots", "GS_GREEDY_SWITCH": "greedy_switch",
    "GS_SITE_SWITCH": "site_switch", "GS_MULTI_BATCH_FILL": "multi_batch_fill",
    "GS_SWEEP_ONE": "sweep_one",
}


def tuning_spec(spec: str) -> dict:
    """'GS_SITE_COOP=0,greedy_waves=4' -> {'site_coop': 0.0, 'greedy_waves': 4.0}."""
    out = {}
    for kv in filter(None, spec.split(",")):
        k, v = kv.split("=", 1)
        out[TUNING_ALIASES.get(k, k)] = float(v)
    return out


class GibbsError(RuntimeError):
    """Base error; `.status` is the gs_status, `.index` the failing sequence."""

    def __init__(self, status: int, msg: str, index: int = -1):
        super().__init__(f"[gs_status {status}] {msg}" + (f" (sequence {index})" if index >= 0 else ""))
        self.status = status
        self.index = index


class ArgumentError(GibbsError, ValueError):
    """.NET ArgumentOutOfRangeException / ArgumentException equivalent."""


class RouletteOverrunError(GibbsError, IndexError):
    """The list-index ArgumentException of rouletteWheelSelection (.fs:752)."""


class ChecksumOverflowError(GibbsError, OverflowError):
    """Checked Array.sum overflow (.fs:117)."""


class DeviceError(GibbsError):
    """HIP / RCCL failure (InvalidOperationException in the F# shim)."""


_ERRORS = {
    GS_E_ARG: ArgumentError,
    GS_E_ROULETTE_OVERRUN: RouletteOverrunError,
    GS_E_OVERFLOW: ChecksumOverflowError,
}

_lib = None


def load_library(path: str | os.PathLike | None = None) -> C.CDLL:
    """Load libgibbs_hip.so (fails loudly when it is absent)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path).resolve() if path else LIB_PATH
    if not p.exists():
        raise ImportError(
            f"{p} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the HIP path has no CPU fallback)")
    # One HIP runtime per process: when PyTorch is present it must be loaded first so
    # that libgibbs_hip.so binds to torch's libamdhip64.so.7 / librccl (same SONAMEs)
    # instead of pulling /opt/rocm's copies in beside them (two runtimes abort at exit).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(str(p), mode=C.RTLD_LOCAL)
    # (an explicit path may name an older build kept for A/B runs: entry points it
    # lacks stay undeclared there; the shipped library must export every one)
    _declare(lib, strict=path is None)
    if path is None:
        _lib = lib
    return lib


def _declare(lib: C.CDLL, strict: bool = True) -> None:
    vp, i32, i64, u64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double
    P = C.POINTER
    sig = {
        "gs_create": (C.c_int, [i32, P(vp)]),
        "gs_destroy": (C.c_int, [vp]),
        "gs_set_tuning": (C.c_int, [vp, C.c_char_p, f64]),
        "gs_get_tuning": (C.c_int, [vp, C.c_char_p, P(f64)]),
        "gs_last_error": (C.c_char_p, [vp]),
        "gs_error_index": (i64, [vp]),
        "gs_version": (C.c_char_p, []),
        "gs_set_sequences": (C.c_int, [vp, vp, vp, i32, vp, i32, i64, i64]),
        "gs_comm_unique_id": (C.c_int, [vp]),
        "gs_comm_init": (C.c_int, [vp, vp, i32, i32]),
        "gs_motif_sweep": (C.c_int, [vp, i32, f64, f64, vp, vp, vp, vp]),
        "gs_state_set_positions": (C.c_int, [vp, i32, vp]),
        "gs_run_sweeps": (C.c_int, [vp, f64, f64, i32, u64, i64]),
        "gs_state_get": (C.c_int, [vp, vp, vp]),
        "gs_prepare_sweeps": (C.c_int, [vp, f64, f64, u64]),
        "gs_synchronize": (C.c_int, [vp]),
        "gs_motif_run": (C.c_int, [vp, i32, f64, f64, i32, u64, i64, vp, vp]),
        "gs_run_greedy": (C.c_int, [vp, f64, f64, i32, P(i32), P(f64)]),
        "gs_motif_greedy": (C.c_int, [vp, i32, f64, f64, i32, vp, vp, P(i32)]),
        "gs_motif_sampling": (C.c_int, [vp, i32, f64, f64, u64, i32, i32, vp, vp, P(i32)]),
        "gs_motif_sampling_batch": (C.c_int, [vp, i32, f64, f64, vp, i32, i32, i32, vp, vp, vp,
                                              vp]),
        "gs_motif_sampling_batch_fixed": (C.c_int, [vp, i32, f64, f64, vp, vp, vp, i32, i32, i32,
                                                    vp, vp, vp, vp]),
        "gs_batch_last_ms": (C.c_int, [vp, vp]),
        "gs_motif_sweep_multi": (C.c_int, [vp, i32, i32, f64, f64, i32, vp, vp, vp, vp, vp, vp]),
        "gs_motif_greedy_multi": (C.c_int, [vp, i32, i32, f64, f64, i32, i32, vp, vp, vp,
                                            P(i32)]),
        "gs_motif_sampling_multi": (C.c_int, [vp, i32, i32, f64, f64, u64, i32, i32, i32, vp, vp,
                                              vp, P(i32)]),
        "gs_motif_sampling_multi_batch": (C.c_int, [vp, i32, i32, f64, f64, vp, i32, i32, i32, i32,
                                                    vp, vp, vp, vp, vp]),
        "gs_motif_sampling_multi_batch_fixed": (C.c_int, [vp, i32, i32, f64, f64, vp, vp, vp, i32,
                                                          i32, i32, i32, vp, vp, vp, vp, vp]),
        "gs_multi_batch_last_ms": (C.c_int, [vp, vp]),
        "gs_multi_batch_last_info": (C.c_int, [vp, vp]),
        "gs_motif_run_batch": (C.c_int, [vp, i32, f64, f64, i32, vp, i32, i64, i32, vp, vp, vp,
                                         vp]),
        "gs_run_batch_last_ms": (C.c_int, [vp, vp]),
        "gs_occupancy_size": (i64, [vp, i32]),
        "gs_occupancy_offsets": (C.c_int, [vp, i32, vp]),
        "gs_motif_run_batch_stats": (C.c_int, [vp, i32, f64, f64, i32, vp, i32, i64, i32, vp, i32,
                                               i32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "gs_run_sweeps_stats": (C.c_int, [vp, f64, f64, i32, u64, i64, vp, i32, i32, vp, vp, vp, vp,
                                          vp]),
        "gs_motif_run_stats": (C.c_int, [vp, i32, f64, f64, i32, u64, i64, vp, i32, i32, vp, vp, vp,
                                         vp, vp, vp, vp]),
        "gs_run_stats_last_ms": (C.c_int, [vp, vp]),
        "gs_occupancy_summary": (C.c_int, [vp, i32, vp, i32, i64, vp, vp, vp, vp, vp, vp, vp]),
        "gs_run_sweeps_summary": (C.c_int, [vp, f64, f64, i32, u64, i64, vp, i32, i32, vp, vp, vp,
                                            vp, vp, vp, vp, vp]),
        "gs_motif_run_summary": (C.c_int, [vp, i32, f64, f64, i32, u64, i64, vp, i32, i32, vp, vp,
                                           vp, vp, vp, vp, vp, vp, vp, vp]),
        "gs_motif_run_batch_summary": (C.c_int, [vp, i32, f64, f64, i32, vp, i32, i64, i32, vp, i32,
                                                 i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                 vp, vp, vp]),
        "gs_summary_last_ms": (C.c_int, [vp, vp]),
        "gs_occupancy_agreement": (C.c_int, [vp, i32, vp, i32, i64, vp, vp, vp, vp, vp, vp, vp]),
        "gs_motif_run_batch_agreement": (C.c_int, [vp, i32, f64, f64, i32, vp, i32, i64, i32, vp,
                                                   i32, i32] + [vp] * 21),
        "gs_agreement_last_ms": (C.c_int, [vp, vp]),
        "gs_state_motif_length": (i32, [vp]),
        "gs_motif_run_multi_batch": (C.c_int, [vp, i32, i32, f64, f64, i32, vp, i32, i64, i32, i32,
                                               vp, vp, vp, vp, vp]),
        "gs_motif_run_multi_batch_stats": (C.c_int, [vp, i32, i32, f64, f64, i32, vp, i32, i64, i32,
                                                     i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp,
                                                     vp, vp, vp, vp]),
        "gs_list_occupancy_summary": (C.c_int, [vp, i32, i32, vp, vp, i32, i64] + [vp] * 13),
        "gs_motif_run_multi_batch_summary": (C.c_int, [vp, i32, i32, f64, f64, i32, vp, i32, i64,
                                                       i32, i32, vp, i32, i32] + [vp] * 24),
        "gs_motif_run_multi": (C.c_int, [vp, i32, i32, f64, f64, i32, u64, i64, i32, vp, vp, vp]),
        "gs_run_multi_batch_last_ms": (C.c_int, [vp, vp]),
        "gs_run_multi_batch_last_info": (C.c_int, [vp, vp]),
        "gs_set_fixed_pcv": (C.c_int, [vp, vp]),
        "gs_set_fixed_ppm": (C.c_int, [vp, vp, i32]),
        "gs_site_scan": (C.c_int, [vp, i32, f64, vp, vp, vp]),
        "gs_site_refine": (C.c_int, [vp, i32, f64, i32, i32, vp, vp, P(i32)]),
        "gs_site_sampling": (C.c_int, [vp, i32, f64, u64, i32, i32, vp, vp, vp]),
        "gs_site_sampling_batch": (C.c_int, [vp, i32, f64, vp, i32, i32, i32, vp, vp, vp, vp]),
        "gs_site_sampling_batch_fixed": (C.c_int, [vp, i32, f64, vp, vp, vp, i32, i32, i32, vp, vp,
                                                   vp, vp]),
        "gs_site_batch_last_ms": (C.c_int, [vp, vp]),
        "gs_counts": (C.c_int, [vp, i32, vp, vp, vp]),
        "gs_random_starts": (C.c_int, [vp, i32, f64, u64, i32, vp, vp]),
        "gs_random_starts_batch": (C.c_int, [vp, i32, f64, vp, i32, i32, vp, vp, vp]),
        "gs_starts_batch_last_ms": (C.c_int, [vp, vp]),
        "gs_best_pwms": (C.c_int, [vp, i32, f64, i32, vp, vp, P(f64), P(i32)]),
        "gs_uniform": (f64, [u64, u64, u64]),
        "gs_stream_sweep": (u64, [u64]),
        "gs_profile_enable": (C.c_int, [vp, i32]),
        "gs_profile_read": (C.c_int, [vp, P(f64), P(i64), P(f64), P(i64)]),
        "gs_profile_region_begin": (C.c_int, [vp]),
        "gs_profile_region_end": (C.c_int, [vp, P(f64)]),
        "gs_profile_region_stop": (C.c_int, [vp]),
        "gs_stats": (C.c_int, [vp, vp, i32]),
        "gs_sweep_kernel_name": (C.c_char_p, [vp]),
        "gs_last_sweep_launch": (C.c_int, [vp, vp]),
        "gs_last_sweep_one": (C.c_int, [vp]),
        "gs_set_scan_mode": (C.c_int, [vp, i32]),
        "gs_fastmath_check": (C.c_int, [vp, P(f64), P(f64)]),
        "gs_agg_size": (i64, [vp]),
        "gs_agg_download": (C.c_int, [vp, vp]),
        "gs_agg_upload": (C.c_int, [vp, vp]),
        "gs_exchange_handle": (C.c_int, [vp, vp]),
        "gs_exchange_open": (C.c_int, [vp, vp, i32, i32]),
        "gs_exchange_close": (C.c_int, [vp]),
    }
    for name, (res, args) in sig.items():
        if not strict and not hasattr(lib, name):
            continue
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args


def header_symbols(header: Path = HEADER_PATH) -> list[str]:
    """Every function declared in include/gibbs_hip.h."""
    text = header.read_text()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[\w\s\*]+?\b(gs_\w+)\s*\(", text, re.M)))


def _ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def fixed_args(pcv, ppm, W: int):
    """The pcv= / ppm= keywords of the batched drivers as contiguous float64 arrays (None
    stays None): 49 CompositeVector slots, 49 slot rows x W columns.  A wrong shape raises
    ArgumentError before any native call."""
    if pcv is not None:
        pcv = np.ascontiguousarray(pcv, np.float64)
        if pcv.shape != (49,):
            raise ArgumentError(GS_E_ARG, "pcv needs the 49 CompositeVector slots")
    if ppm is not None:
        ppm = np.ascontiguousarray(ppm, np.float64)
        if ppm.shape != (49, int(W)):
            raise ArgumentError(GS_E_ARG, "ppm needs 49 slot rows x motifLength columns")
    return pcv, ppm


class Context:
    """One gs_ctx: one GPU, one shard of the sequences."""

    def __init__(self, device: int = 0, lib_path: str | os.PathLike | None = None,
                 tuning: dict | None = None):
        self.lib = load_library(lib_path)
        h = C.c_void_p()
        st = self.lib.gs_create(int(device), C.byref(h))
        if st != GS_OK:
            raise DeviceError(st, f"gs_create(device={device}) failed")
        self.h = h
        self.n_local = 0
        self.lengths = np.zeros(0, np.int64)
        for k, v in (tuning or {}).items():
            self.set_tuning(k, v)

    def set_tuning(self, name: str, value: float) -> None:
        """Engine tuning field (gs_set_tuning: diagnostics and A/B runs; the results
        never depend on it).  Set before set_sequences."""
        self._check(self.lib.gs_set_tuning(self.h, name.encode(), C.c_double(float(value))))

    def get_tuning(self, name: str) -> float:
        v = C.c_double()
        self._check(self.lib.gs_get_tuning(self.h, name.encode(), C.byref(v)))
        return v.value

    # -- plumbing
    def close(self) -> None:
        if self.h:
            self.lib.gs_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st: int) -> None:
        if st == GS_OK:
            return
        msg = (self.lib.gs_last_error(self.h) or b"").decode(errors="replace")
        idx = int(self.lib.gs_error_index(self.h))
        raise _ERRORS.get(st, DeviceError)(st, msg, idx)

    # -- data
    def set_sequences(self, codes: np.ndarray, offsets: np.ndarray, alphabet: bytes | np.ndarray,
                      n_global: int | None = None, global_offset: int = 0) -> None:
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        alpha = np.frombuffer(bytes(alphabet), np.uint8) if isinstance(alphabet, (bytes, bytearray)) \
            else np.ascontiguousarray(alphabet, dtype=np.uint8)
        n = len(offsets) - 1
        ng = n if n_global is None else int(n_global)
        self._check(self.lib.gs_set_sequences(self.h, _ptr(codes), _ptr(offsets), n, _ptr(alpha),
                                              len(alpha), ng, int(global_offset)))
        self.n_local = n
        self.lengths = np.diff(offsets)
        self._keep = (codes, offsets, alpha)

    def comm_init(self, unique_id: bytes, nranks: int, rank: int) -> None:
        buf = (C.c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        self._check(self.lib.gs_comm_init(self.h, buf, int(nranks), int(rank)))

    @staticmethod
    def unique_id() -> bytes:
        lib = load_library()
        buf = (C.c_uint8 * UNIQUE_ID_BYTES)()
        st = lib.gs_comm_unique_id(buf)
        if st != GS_OK:
            raise DeviceError(st, "gs_comm_unique_id failed")
        return bytes(buf)

    # -- hot path
    def motif_sweep(self, W: int, pc: float, cutoff: float, pos_in, u):
        pos_in = np.ascontiguousarray(pos_in, dtype=np.int32)
        u = np.ascontiguousarray(u, dtype=np.float64)
        if pos_in.shape != (self.n_local,) or u.shape != (self.n_local,):
            raise ArgumentError(GS_E_ARG, "pos_in and u need one entry per sequence")
        pos_out = np.empty(self.n_local, np.int32)
        pwms = np.empty(self.n_local, np.float64)
        self._check(self.lib.gs_motif_sweep(self.h, int(W), float(pc), float(cutoff), _ptr(pos_in),
                                            _ptr(u), _ptr(pos_out), _ptr(pwms)))
        return pos_out, pwms

    def set_positions(self, W: int, pos) -> None:
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        self._check(self.lib.gs_state_set_positions(self.h, int(W), _ptr(pos)))

    def run_sweeps(self, pc: float, cutoff: float, n_sweeps: int, seed: int, first_sweep: int = 0):
        self._check(self.lib.gs_run_sweeps(self.h, float(pc), float(cutoff), int(n_sweeps),
                                           int(seed) & (2**64 - 1), int(first_sweep)))

    def prepare_sweeps(self, pc: float, cutoff: float, seed: int) -> None:
        """Capture the sweep-chain graph for the current phase ahead of time."""
        self._check(self.lib.gs_prepare_sweeps(self.h, float(pc), float(cutoff),
                                               int(seed) & (2**64 - 1)))

    def get_state(self):
        pos = np.empty(self.n_local, np.int32)
        pwms = np.empty(self.n_local, np.float64)
        self._check(self.lib.gs_state_get(self.h, _ptr(pos), _ptr(pwms)))
        return pos, pwms

    def synchronize(self) -> None:
        self._check(self.lib.gs_synchronize(self.h))

    def motif_run(self, W, pc, cutoff, n_sweeps, seed, pos, first_sweep=0):
        pos = np.array(pos, dtype=np.int32, copy=True)
        pwms = np.empty(self.n_local, np.float64)
        self._check(self.lib.gs_motif_run(self.h, int(W), float(pc), float(cutoff), int(n_sweeps),
                                          int(seed) & (2**64 - 1), int(first_sweep), _ptr(pos),
                                          _ptr(pwms)))
        return pos, pwms

    def run_greedy(self, pc: float, cutoff: float, max_passes: int = 1000):
        """Greedy refinement of the resident snapshot (.fs:885-929); returns
        (passes, kernel milliseconds)."""
        passes, ms = C.c_int32(0), C.c_double(0.0)
        self._check(self.lib.gs_run_greedy(self.h, float(pc), float(cutoff), int(max_passes),
                                           C.byref(passes), C.byref(ms)))
        return passes.value, ms.value

    def motif_greedy(self, W: int, pc: float, cutoff: float, pos, pwms, max_passes: int = 1000):
        """findBestMotifIndicesWithStartPositions on (pos, pwms) = motifMem; returns
        (pos, pwms, passes)."""
        pos = np.array(pos, dtype=np.int32, copy=True)
        pwms = np.array(pwms, dtype=np.float64, copy=True)
        if pos.shape != (self.n_local,) or pwms.shape != (self.n_local,):
            raise ArgumentError(GS_E_ARG, "pos and pwms need one entry per sequence")
        passes = C.c_int32(0)
        self._check(self.lib.gs_motif_greedy(self.h, int(W), float(pc), float(cutoff),
                                             int(max_passes), _ptr(pos), _ptr(pwms),
                                             C.byref(passes)))
        return pos, pwms, passes.value

    def motif_sampling(self, W: int, pc: float, cutoff: float, seed: int, init_mode: int = 0,
                       max_passes: int = 1000):
        """doMotifSampling (.fs:1034-1038) on the device -> (pos, pwms, greedy passes)."""
        pos = np.empty(self.n_local, np.int32)
        pwms = np.empty(self.n_local, np.float64)
        passes = C.c_int32(0)
        self._check(self.lib.gs_motif_sampling(self.h, int(W), float(pc), float(cutoff),
                                               int(seed) & (2**64 - 1), int(init_mode),
                                               int(max_passes), _ptr(pos), _ptr(pwms),
                                               C.byref(passes)))
        return pos, pwms, passes.value

    def motif_sampling_batch(self, W: int, pc: float, cutoff: float, seeds, init_mode: int = 0,
                             max_passes: int = 1000, *, pcv=None, ppm=None):
        """R independent doMotifSampling runs in one call, row r exactly
        motif_sampling(W, pc, cutoff, seeds[r], ...): the chains' greedy passes run
        as R concurrent workgroups -> (pos[R, N], pwms[R, N], passes[R], status[R]).
        A chain that raises (status[r] != 0, e.g. GS_E_OVERFLOW) leaves the other rows
        valid; errors of the call itself raise.  pcv (49 slots) / ppm (49 x W): the
        ByPCV / WithPPM twins (gs_motif_sampling_batch_fixed), row r what motif_sampling
        gives on a context with set_fixed_pcv(pcv) / set_fixed_ppm(ppm)."""
        pcv, ppm = fixed_args(pcv, ppm, W)
        seeds = np.array([int(s) & (2**64 - 1) for s in seeds], dtype=np.uint64)
        R = len(seeds)
        pos = np.empty((R, self.n_local), np.int32)
        pwms = np.empty((R, self.n_local), np.float64)
        passes = np.zeros(R, np.int32)
        status = np.zeros(R, np.int32)
        if pcv is None and ppm is None:
            st = self.lib.gs_motif_sampling_batch(self.h, int(W), float(pc), float(cutoff),
                                                  _ptr(seeds), R, int(init_mode), int(max_passes),
                                                  _ptr(pos), _ptr(pwms), _ptr(passes),
                                                  _ptr(status))
        else:
            st = self.lib.gs_motif_sampling_batch_fixed(
                self.h, int(W), float(pc), float(cutoff), _ptr(pcv), _ptr(ppm), _ptr(seeds), R,
                int(init_mode), int(max_passes), _ptr(pos), _ptr(pwms), _ptr(passes),
                _ptr(status))
        if st != GS_OK and not status.any():
            self._check(st)
        return pos, pwms, passes, status

    def batch_last_ms(self):
        """Device milliseconds of the last motif_sampling_batch: (first stages, greedy launch)."""
        out = np.zeros(2, np.float64)
        self._check(self.lib.gs_batch_last_ms(self.h, _ptr(out)))
        return float(out[0]), float(out[1])

    # -- motifAmount >= 1 with Positions lists
    def _lists(self, cnt, pos, cap):
        cnt = np.array(cnt, dtype=np.int32, copy=True)
        pos = np.array(pos, dtype=np.int32, copy=True).reshape(self.n_local, cap)
        if cnt.shape != (self.n_local,):
            raise ArgumentError(GS_E_ARG, "cnt needs one entry per sequence")
        return cnt, np.ascontiguousarray(pos)

    def motif_sweep_multi(self, motif_amount: int, W: int, pc: float, cutoff: float, cnt, pos, u,
                          cap: int | None = None):
        """findBestMotifIndicesByWithStartPositions (.fs:935-970) with Positions lists:
        (cnt[n], pos[n, :cnt[n]]) in F# list order -> (cnt, pos[N, cap], pwms)."""
        cap = int(cap or motif_amount)
        cnt, pos = self._lists(cnt, pos, cap)
        u = np.ascontiguousarray(u, dtype=np.float64)
        if u.shape != (self.n_local,):
            raise ArgumentError(GS_E_ARG, "u needs one entry per sequence")
        co = np.empty(self.n_local, np.int32)
        po = np.full((self.n_local, cap), -1, np.int32)
        pw = np.empty(self.n_local, np.float64)
        self._check(self.lib.gs_motif_sweep_multi(self.h, int(motif_amount), int(W), float(pc),
                                                  float(cutoff), cap, _ptr(cnt), _ptr(pos), _ptr(u),
                                                  _ptr(co), _ptr(po), _ptr(pw)))
        return co, po, pw

    def motif_greedy_multi(self, motif_amount: int, W: int, pc: float, cutoff: float, cnt, pos,
                           pwms, max_passes: int = 1000, cap: int | None = None):
        """findBestMotifIndicesWithStartPositions (.fs:885-929) with Positions lists ->
        (cnt, pos[N, cap], pwms, passes)."""
        cap = int(cap or motif_amount)
        cnt, pos = self._lists(cnt, pos, cap)
        pwms = np.array(pwms, dtype=np.float64, copy=True)
        passes = C.c_int32(0)
        self._check(self.lib.gs_motif_greedy_multi(self.h, int(motif_amount), int(W), float(pc),
                                                   float(cutoff), int(max_passes), cap, _ptr(cnt),
                                                   _ptr(pos), _ptr(pwms), C.byref(passes)))
        return cnt, pos, pwms, passes.value

    def motif_sampling_multi(self, motif_amount: int, W: int, pc: float, cutoff: float, seed: int,
                             init_mode: int = 0, max_passes: int = 1000, cap: int | None = None):
        """doMotifSampling (.fs:1034-1038) with any motifAmount ->
        (cnt, pos[N, cap], pwms, greedy passes)."""
        cap = int(cap or motif_amount)
        co = np.empty(self.n_local, np.int32)
        po = np.full((self.n_local, cap), -1, np.int32)
        pw = np.empty(self.n_local, np.float64)
        passes = C.c_int32(0)
        self._check(self.lib.gs_motif_sampling_multi(self.h, int(motif_amount), int(W), float(pc),
                                                     float(cutoff), int(seed) & (2**64 - 1),
                                                     int(init_mode), int(max_passes), cap,
                                                     _ptr(co), _ptr(po), _ptr(pw),
                                                     C.byref(passes)))
        return co, po, pw, passes.value

    def motif_sampling_multi_batch(self, motif_amount: int, W: int, pc: float, cutoff: float,
                                   seeds, init_mode: int = 0, max_passes: int = 1000,
                                   cap: int | None = None, *, pcv=None, ppm=None):
        """R independent doMotifSampling runs with any motifAmount in one call, row r
        exactly motif_sampling_multi(motif_amount, W, pc, cutoff, seeds[r], ...): sweep 0
        over all (chain, target) pairs at once, the chains' greedy passes side by side ->
        (cnt[R, N], pos[R, N, cap], pwms[R, N], passes[R], status[R]).  A chain that
        raises (status[r] != 0, e.g. GS_E_OVERFLOW) leaves the other rows valid; errors
        of the call itself raise.  pcv (49 slots) / ppm (49 x W): the ByPCV / WithPPM twins
        (gs_motif_sampling_multi_batch_fixed), row r what motif_sampling_multi gives on a
        context with set_fixed_pcv(pcv) / set_fixed_ppm(ppm)."""
        pcv, ppm = fixed_args(pcv, ppm, W)
        cap = int(cap or motif_amount)
        seeds = np.array([int(s) & (2**64 - 1) for s in seeds], dtype=np.uint64)
        R = len(seeds)
        cnt = np.zeros((R, self.n_local), np.int32)
        pos = np.full((R, self.n_local, max(cap, 0)), -1, np.int32)
        pwms = np.zeros((R, self.n_local), np.float64)
        passes = np.zeros(R, np.int32)
        status = np.zeros(R, np.int32)
        if pcv is None and ppm is None:
            st = self.lib.gs_motif_sampling_multi_batch(
                self.h, int(motif_amount), int(W), float(pc), float(cutoff), _ptr(seeds), R,
                int(init_mode), int(max_passes), cap, _ptr(cnt), _ptr(pos), _ptr(pwms),
                _ptr(passes), _ptr(status))
        else:
            st = self.lib.gs_motif_sampling_multi_batch_fixed(
                self.h, int(motif_amount), int(W), float(pc), float(cutoff), _ptr(pcv), _ptr(ppm),
                _ptr(seeds), R, int(init_mode), int(max_passes), cap, _ptr(cnt), _ptr(pos),
                _ptr(pwms), _ptr(passes), _ptr(status))
        if st != GS_OK and not status.any():
            self._check(st)
        return cnt, pos, pwms, passes, status

    def multi_batch_last_ms(self):
        """Device milliseconds of the last motif_sampling_multi_batch: (starts, sweep,
        greedy passes)."""
        out = np.zeros(3, np.float64)
        self._check(self.lib.gs_multi_batch_last_ms(self.h, _ptr(out)))
        return float(out[0]), float(out[1]), float(out[2])

    def multi_batch_last_info(self) -> dict:
        """Rounds of the last motif_sampling_multi_batch: sweep rounds after the first
        (arena growth), greedy restart rounds, chains restarted in all, speculative slots
        per chain of the first greedy round."""
        out = np.zeros(4, np.int32)
        self._check(self.lib.gs_multi_batch_last_info(self.h, _ptr(out)))
        return dict(zip(("sweep_rounds", "restart_rounds", "chains_restarted", "slots"),
                        (int(v) for v in out)))

    def _run_batch_args(self, n_sweeps, seeds, pos, init_mode, u):
        """The chains' seeds, starts and uniforms as the library takes them (motif_run_batch and
        its _stats and _summary forms) -> (seeds, pos, init_mode, u)."""
        seeds = np.array([int(s) & (2**64 - 1) for s in seeds], dtype=np.uint64)
        R = len(seeds)
        if pos is not None:
            init_mode = -1
            pos = np.array(pos, dtype=np.int32, copy=True)
            if pos.shape != (R, self.n_local):
                raise ArgumentError(GS_E_ARG, "pos needs one row per seed, one entry per sequence")
        else:
            if init_mode not in (0, 1):
                raise ArgumentError(GS_E_ARG, "init_mode must be 0 or 1 when no starts are given")
            pos = np.full((R, self.n_local), -1, np.int32)
        if u is not None:
            u = np.ascontiguousarray(u, dtype=np.float64)
            if u.shape != (R, max(int(n_sweeps), 0), self.n_local):
                raise ArgumentError(GS_E_ARG, "u needs the shape [chains, sweeps, sequences]")
        return seeds, pos, init_mode, u

    @staticmethod
    def _n_counted(burn_in, thin, n_sweeps):
        """The counted sweeps of a chain (out-of-range values go to the library, which refuses
        them: the shapes are then moot)."""
        ok = 0 <= burn_in <= n_sweeps and thin >= 1
        return len(range(burn_in, n_sweeps, thin)) if ok else 0

    def _stats_outputs(self, W, lead, n_counted, occupancy, ic, best, sites=False, M=None,
                       cap=None, H=None):
        """The output arrays of a chain's statistics, the parts asked for, under the leading
        axes `lead` (() or (R,)) -> dict.  W: the motif length the bins are for (None: none can
        be sized), H: their number where the caller has it; M and cap: a list chain's
        motifAmount ("sites") and capacity ("best_cnt", a third axis of "best_pos")."""
        N = self.n_local
        stats = {}
        if occupancy:
            if H is None:
                H = int(self.lib.gs_occupancy_size(self.h, int(W))) if W is not None else -1
            if H >= 0:
                stats["offsets"] = self.occupancy_offsets(W)
            stats["occupancy"] = np.zeros(lead + (max(H, 0),), np.int32)
        if sites:
            stats["sites"] = np.zeros(lead + (N, max(M, 0) + 1), np.int32)
        if ic:
            stats["ic"] = np.full(lead + (n_counted,), np.nan, np.float64)
        if best:
            stats["best_sweep"] = np.full(lead or (1,), -1, np.int64)
            if cap is not None:
                stats["best_cnt"] = np.zeros(lead + (N,), np.int32)
            stats["best_pos"] = np.full(lead + (N,) + (() if cap is None else (max(cap, 0),)), -1,
                                        np.int32)
            stats["best_pwms"] = np.zeros(lead + (N,), np.float64)
        return stats

    def motif_run_batch(self, W: int, pc: float, cutoff: float, n_sweeps: int, seeds, pos=None,
                        init_mode: int = 0, first_sweep: int = 0, u=None, strict: bool = False):
        """R independent chains of n_sweeps sweeps in one call, row r exactly
        motif_run(W, pc, cutoff, n_sweeps, seeds[r], start r, first_sweep): one launch a
        sweep over all (chain, target) pairs -> (pos[R, N], pwms[R, N], status[R]).  The
        starts are the rows of `pos` (-1 = Positions []; implies init_mode -1) or those of
        random_starts(W, pc, seeds[r], init_mode).  u[R, n_sweeps, N] replaces the counter
        RNG's uniforms.  pwms is unspecified for n_sweeps = 0.  A chain that raises
        (status[r] != 0) leaves the other rows valid; errors of the call itself raise, and
        with strict=True so does a chain's (the lowest-index failing chain's status, the
        exception's index its sequence)."""
        seeds, pos, init_mode, u = self._run_batch_args(n_sweeps, seeds, pos, init_mode, u)
        R = len(seeds)
        pwms = np.zeros((R, self.n_local), np.float64)
        status = np.zeros(R, np.int32)
        st = self.lib.gs_motif_run_batch(self.h, int(W), float(pc), float(cutoff), int(n_sweeps),
                                         _ptr(seeds), R, int(first_sweep), int(init_mode), _ptr(u),
                                         _ptr(pos), _ptr(pwms), _ptr(status))
        if st != GS_OK and (strict or not status.any()):
            self._check(st)
        return pos, pwms, status

    def occupancy_offsets(self, W: int) -> np.ndarray:
        """Bins of one chain's occupancy histogram for motif length W, off[N + 1]: sequence
        n owns off[n] .. off[n + 1] - 1, bin off[n] counts Positions [], bin off[n] + 1 + k
        start k; off[N] is the histogram's length H."""
        if int(self.lib.gs_occupancy_size(self.h, int(W))) < 0:
            raise ArgumentError(GS_E_ARG, "occupancy_offsets: a bad motifLength, or no sequences")
        off = np.zeros(self.n_local + 1, np.int64)
        self._check(self.lib.gs_occupancy_offsets(self.h, int(W), _ptr(off)))
        return off

    def motif_run_batch_stats(self, W: int, pc: float, cutoff: float, n_sweeps: int, seeds,
                              pos=None, init_mode: int = 0, first_sweep: int = 0, u=None,
                              burn_in: int = 0, thin: int = 1, occupancy: bool = True,
                              ic: bool = True, best: bool = True, strict: bool = False):
        """motif_run_batch with statistics of the chains' sweeps, gathered on the device
        with no host wait -> (pos[R, N], pwms[R, N], status[R], stats).  Sweep t counts when
        t >= burn_in and (t - burn_in) % thin == 0.  stats is a dict of the parts asked for:
        "occupancy"[R, H] (the counted sweeps whose state has its sequence at that bin,
        occupancy_offsets) with "offsets"[N + 1]; "ic"[R, n_counted], the sum of the PWMS of
        each counted sweep in the fixed order of sampler.informationContent; "best_sweep"[R]
        (first_sweep + t of the first largest ic, -1: none), "best_pos"[R, N] and
        "best_pwms"[R, N].  A chain that raises in sweep t contributes nothing from t on
        (its ic entries are NaN).  With no part asked for this is motif_run_batch."""
        seeds, pos, init_mode, u = self._run_batch_args(n_sweeps, seeds, pos, init_mode, u)
        R, T = len(seeds), int(n_sweeps)
        burn_in, thin = int(burn_in), int(thin)
        pwms = np.zeros((R, self.n_local), np.float64)
        status = np.zeros(R, np.int32)
        stats = self._stats_outputs(W, (R,), self._n_counted(burn_in, thin, T), occupancy, ic, best)
        st = self.lib.gs_motif_run_batch_stats(
            self.h, int(W), float(pc), float(cutoff), T, _ptr(seeds), R, int(first_sweep),
            int(init_mode), _ptr(u), burn_in, thin, _ptr(pos), _ptr(pwms), _ptr(status),
            _ptr(stats.get("occupancy")), _ptr(stats.get("ic")), _ptr(stats.get("best_sweep")),
            _ptr(stats.get("best_pos")), _ptr(stats.get("best_pwms")))
        if st != GS_OK and (strict or not status.any()):
            self._check(st)
        return pos, pwms, status, stats

    def run_batch_last_ms(self):
        """Device milliseconds of the last motif_run_batch or motif_run_batch_stats: (starts
        and their aggregates, sweeps with the statistics launches)."""
        out = np.zeros(2, np.float64)
        self._check(self.lib.gs_run_batch_last_ms(self.h, _ptr(out)))
        return float(out[0]), float(out[1])

    def _chain_stats_outputs(self, W, n_sweeps, u, burn_in, thin, occupancy, ic, best):
        """The uniforms and the output arrays of run_sweeps_stats / motif_run_stats (W: the
        motif length the bins are for, None: none can be sized) -> (u, burn_in, thin, stats)."""
        T = int(n_sweeps)
        if u is not None:
            u = np.ascontiguousarray(u, dtype=np.float64)
            if u.shape != (max(T, 0), self.n_local):
                raise ArgumentError(GS_E_ARG, "u needs the shape [sweeps, sequences]")
        burn_in, thin = int(burn_in), int(thin)
        stats = self._stats_outputs(W, (), self._n_counted(burn_in, thin, T), occupancy, ic, best)
        return u, burn_in, thin, stats

    def run_sweeps_stats(self, pc: float, cutoff: float, n_sweeps: int, seed: int,
                         first_sweep: int = 0, u=None, burn_in: int = 0, thin: int = 1,
                         occupancy: bool = True, ic: bool = True, best: bool = True,
                         strict: bool = True):
        """run_sweeps with statistics of the chain's sweeps, gathered on the device with no
        host wait between sweeps (gs_run_sweeps_stats) -> stats.  The chain starts from the
        resident snapshot (set_positions, a previous chain), whose motif length sizes the bins;
        without one the call raises with status GS_E_STATE.  Sweep t counts when t >= burn_in and
        (t - burn_in) % thin == 0.  stats is a dict of the parts asked for: "occupancy"[H]
        (the counted sweeps whose state has its sequence at that bin) with "offsets"[N + 1];
        "ic"[n_counted], the sum of the PWMS of each counted sweep in the fixed order of
        sampler.informationContent; "best_sweep"[1] (first_sweep + t of the first largest ic,
        -1: none), "best_pos"[N] and "best_pwms"[N]; and "status", the call's gs_status.  u[n_sweeps,
        N] replaces the counter RNG's uniforms.  The snapshot stays on the context (get_state).
        A chain that raises in sweep t counts nothing from t on (its ic entries are NaN) and
        raises here; with strict=False the status is returned in stats instead."""
        W = int(self.lib.gs_state_motif_length(self.h))
        if W <= 0:
            raise DeviceError(GS_E_STATE, "no snapshot: call set_positions")
        u, burn_in, thin, stats = self._chain_stats_outputs(W, n_sweeps, u, burn_in, thin,
                                                            occupancy, ic, best)
        st = self.lib.gs_run_sweeps_stats(
            self.h, float(pc), float(cutoff), int(n_sweeps), int(seed) & (2**64 - 1),
            int(first_sweep), _ptr(u), burn_in, thin, _ptr(stats.get("occupancy")),
            _ptr(stats.get("ic")), _ptr(stats.get("best_sweep")), _ptr(stats.get("best_pos")),
            _ptr(stats.get("best_pwms")))
        if st != GS_OK and (strict or st not in (GS_E_ROULETTE_OVERRUN, GS_E_OVERFLOW)):
            self._check(st)
        stats["status"] = int(st)
        return stats

    def motif_run_stats(self, W: int, pc: float, cutoff: float, n_sweeps: int, seed: int, pos,
                        first_sweep: int = 0, u=None, burn_in: int = 0, thin: int = 1,
                        occupancy: bool = True, ic: bool = True, best: bool = True):
        """motif_run with the statistics of run_sweeps_stats in one call (gs_motif_run_stats)
        -> (pos, pwms, stats)."""
        pos = np.array(pos, dtype=np.int32, copy=True)
        if pos.shape != (self.n_local,):
            raise ArgumentError(GS_E_ARG, "pos needs one entry per sequence")
        pwms = np.zeros(self.n_local, np.float64)
        u, burn_in, thin, stats = self._chain_stats_outputs(W, n_sweeps, u, burn_in, thin,
                                                            occupancy, ic, best)
        self._check(self.lib.gs_motif_run_stats(
            self.h, int(W), float(pc), float(cutoff), int(n_sweeps), int(seed) & (2**64 - 1),
            int(first_sweep), _ptr(u), burn_in, thin, _ptr(pos), _ptr(pwms),
            _ptr(stats.get("occupancy")), _ptr(stats.get("ic")), _ptr(stats.get("best_sweep")),
            _ptr(stats.get("best_pos")), _ptr(stats.get("best_pwms"))))
        stats["status"] = GS_OK
        return pos, pwms, stats

    def run_stats_last_ms(self):
        """Device milliseconds of the last run_sweeps_stats: (the chain of launches, the
        statistics launches); the second is measured only with the profile on, and is then
        taken out of the first."""
        out = np.zeros(2, np.float64)
        self._check(self.lib.gs_run_stats_last_ms(self.h, _ptr(out)))
        return float(out[0]), float(out[1])

    def _summary_cells(self, W):
        """Entries of a summary's count matrix, A W + A (W None: it cannot be sized)."""
        A = len(getattr(self, "_keep", (None, None, ()))[2])  # the alphabet's length
        return A * int(W) + A if W is not None else 0

    def _summary_outputs(self, W, R, modes, counts, pool):
        """The output arrays of a chain summary of R chains (R None: the single chain's,
        without a chain axis) -> dict."""
        lead = () if R is None else (R,)
        cells = self._summary_cells(W)
        out = {}
        if modes:
            out["mode_pos"] = np.full(lead + (self.n_local,), -1, np.int32)
            out["mode_count"] = np.zeros(lead + (self.n_local,), np.int32)
        if counts:
            out["counts"] = np.zeros(lead + (max(cells, 0),), np.int64)
        if pool:
            out["pooled_pos"] = np.full(self.n_local, -1, np.int32)
            out["pooled_count"] = np.zeros(self.n_local, np.int64)
            out["pooled_counts"] = np.zeros(max(cells, 0), np.int64)
            out["n_pooled"] = np.zeros(1, np.int32)
        return out

    def occupancy_summary(self, W: int, occupancy, n_counted: int, modes: bool = True,
                          counts: bool = True, pool: bool = True) -> dict:
        """The reduction of caller-held histograms occupancy[R, H] (occupancy_offsets(W): a
        statistics call's, or the sums of several) on the device (gs_occupancy_summary) ->
        dict of the groups asked for: "mode_pos"[R, N] and "mode_count"[R, N], each
        sequence's first-maximum bin minus one (-1 = Positions []) and its count;
        "counts"[R, A W + A], the count matrix summed over the counted states in counts()'
        layout, C then T; and, pooled over the chains whose sequence 0 has n_counted counts,
        "pooled_pos"[N], "pooled_count"[N] (int64), "pooled_counts"[A W + A] and
        "n_pooled"[1]."""
        occ = np.ascontiguousarray(occupancy, dtype=np.int32)
        H = int(self.lib.gs_occupancy_size(self.h, int(W)))
        if occ.ndim != 2 or (H >= 0 and occ.shape[1] != H):
            raise ArgumentError(GS_E_ARG, "occupancy needs the shape [chains, bins]")
        R = occ.shape[0]
        out = self._summary_outputs(W if H >= 0 else None, R, modes, counts, pool)
        self._check(self.lib.gs_occupancy_summary(
            self.h, int(W), _ptr(occ) if R > 0 else None, R, int(n_counted),
            _ptr(out.get("mode_pos")), _ptr(out.get("mode_count")), _ptr(out.get("counts")),
            _ptr(out.get("pooled_pos")), _ptr(out.get("pooled_count")),
            _ptr(out.get("pooled_counts")), _ptr(out.get("n_pooled"))))
        return out

    def run_sweeps_summary(self, pc: float, cutoff: float, n_sweeps: int, seed: int,
                           first_sweep: int = 0, u=None, burn_in: int = 0, thin: int = 1,
                           occupancy: bool = False, ic: bool = True, best: bool = True,
                           modes: bool = True, counts: bool = True, strict: bool = True):
        """run_sweeps_stats with the chain's summary reduced on the device behind the last
        statistics launch (gs_run_sweeps_summary) -> stats, with "mode_pos"[N],
        "mode_count"[N] and "counts"[A W + A] as in occupancy_summary.  The bins are
        downloaded only with occupancy=True."""
        W = int(self.lib.gs_state_motif_length(self.h))
        if W <= 0:
            raise DeviceError(GS_E_STATE, "no snapshot: call set_positions")
        u, burn_in, thin, stats = self._chain_stats_outputs(W, n_sweeps, u, burn_in, thin,
                                                            occupancy, ic, best)
        stats.update(self._summary_outputs(W, None, modes, counts, False))
        st = self.lib.gs_run_sweeps_summary(
            self.h, float(pc), float(cutoff), int(n_sweeps), int(seed) & (2**64 - 1),
            int(first_sweep), _ptr(u), burn_in, thin, _ptr(stats.get("occupancy")),
            _ptr(stats.get("ic")), _ptr(stats.get("best_sweep")), _ptr(stats.get("best_pos")),
            _ptr(stats.get("best_pwms")), _ptr(stats.get("mode_pos")),
            _ptr(stats.get("mode_count")), _ptr(stats.get("counts")))
        if st != GS_OK and (strict or st not in (GS_E_ROULETTE_OVERRUN, GS_E_OVERFLOW)):
            self._check(st)
        stats["status"] = int(st)
        return stats

    def motif_run_summary(self, W: int, pc: float, cutoff: float, n_sweeps: int, seed: int, pos,
                          first_sweep: int = 0, u=None, burn_in: int = 0, thin: int = 1,
                          occupancy: bool = False, ic: bool = True, best: bool = True,
                          modes: bool = True, counts: bool = True):
        """motif_run_stats with the summary of run_sweeps_summary in one call
        (gs_motif_run_summary) -> (pos, pwms, stats)."""
        pos = np.array(pos, dtype=np.int32, copy=True)
        if pos.shape != (self.n_local,):
            raise ArgumentError(GS_E_ARG, "pos needs one entry per sequence")
        pwms = np.zeros(self.n_local, np.float64)
        u, burn_in, thin, stats = self._chain_stats_outputs(W, n_sweeps, u, burn_in, thin,
                                                            occupancy, ic, best)
        ok = int(self.lib.gs_occupancy_size(self.h, int(W))) >= 0
        stats.update(self._summary_outputs(W if ok else None, None, modes, counts, False))
        self._check(self.lib.gs_motif_run_summary(
            self.h, int(W), float(pc), float(cutoff), int(n_sweeps), int(seed) & (2**64 - 1),
            int(first_sweep), _ptr(u), burn_in, thin, _ptr(pos), _ptr(pwms),
            _ptr(stats.get("occupancy")), _ptr(stats.get("ic")), _ptr(stats.get("best_sweep")),
            _ptr(stats.get("best_pos")), _ptr(stats.get("best_pwms")),
            _ptr(stats.get("mode_pos")), _ptr(stats.get("mode_count")), _ptr(stats.get("counts"))))
        stats["status"] = GS_OK
        return pos, pwms, stats

    def motif_run_batch_summary(self, W: int, pc: float, cutoff: float, n_sweeps: int, seeds,
                                pos=None, init_mode: int = 0, first_sweep: int = 0, u=None,
                                burn_in: int = 0, thin: int = 1, occupancy: bool = False,
                                ic: bool = True, best: bool = True, modes: bool = True,
                                counts: bool = True, pool: bool = True, strict: bool = False):
        """motif_run_batch_stats with the chains' summaries and the pooled one reduced on the
        device (gs_motif_run_batch_summary) -> (pos[R, N], pwms[R, N], status[R], stats), stats
        with the groups of occupancy_summary besides those of motif_run_batch_stats.  The bins
        are downloaded only with occupancy=True."""
        seeds, pos, init_mode, u = self._run_batch_args(n_sweeps, seeds, pos, init_mode, u)
        R, T = len(seeds), int(n_sweeps)
        burn_in, thin = int(burn_in), int(thin)
        n_counted = self._n_counted(burn_in, thin, T)
        pwms = np.zeros((R, self.n_local), np.float64)
        status = np.zeros(R, np.int32)
        H = int(self.lib.gs_occupancy_size(self.h, int(W)))
        stats = self._stats_outputs(W, (R,), n_counted, occupancy, ic, best, H=H)
        stats.update(self._summary_outputs(W if H >= 0 else None, R, modes, counts, pool))
        st = self.lib.gs_motif_run_batch_summary(
            self.h, int(W), float(pc), float(cutoff), T, _ptr(seeds), R, int(first_sweep),
            int(init_mode), _ptr(u), burn_in, thin, _ptr(pos), _ptr(pwms), _ptr(status),
            _ptr(stats.get("occupancy")), _ptr(stats.get("ic")), _ptr(stats.get("best_sweep")),
            _ptr(stats.get("best_pos")), _ptr(stats.get("best_pwms")),
            _ptr(stats.get("mode_pos")), _ptr(stats.get("mode_count")), _ptr(stats.get("counts")),
            _ptr(stats.get("pooled_pos")), _ptr(stats.get("pooled_count")),
            _ptr(stats.get("pooled_counts")), _ptr(stats.get("n_pooled")))
        if st != GS_OK and (strict or not status.any()):
            self._check(st)
        stats["n_counted"] = n_counted
        return pos, pwms, status, stats

    def summary_last_ms(self) -> float:
        """Device milliseconds of the last chain summary's reduction."""
        out = np.zeros(1, np.float64)
        self._check(self.lib.gs_summary_last_ms(self.h, _ptr(out)))
        return float(out[0])

    def _agreement_outputs(self, R):
        """The output arrays of a chain agreement of R chains -> dict."""
        return {"agree": np.zeros(self.n_local, np.int32),
                "spread": np.zeros(self.n_local, np.int64),
                "spread_chain": np.full(self.n_local, -1, np.int32),
                "chain_agree": np.full(R, -1, np.int32),
                "chain_dist": np.full(R, -1, np.int64),
                "agree_n_pooled": np.zeros(1, np.int32)}

    _AGREEMENT = ("agree", "spread", "spread_chain", "chain_agree", "chain_dist", "agree_n_pooled")

    def occupancy_agreement(self, W: int, occupancy, n_counted: int, pooled=None) -> dict:
        """Whether the chains of caller-held histograms occupancy[R, H] (occupancy_offsets(W))
        agree with their pool, on the device (gs_occupancy_agreement) -> dict.  With P pooled
        chains and pool the sum of their bins, D(r, n) is the sum over sequence n's bins of
        |P occupancy[r] - pool|: D / (2 P n_counted) is the total variation distance between
        the chain's marginal of the sequence and the pooled one.  "agree"[N]: the pooled chains
        whose first-maximum bin of the sequence is the pool's; "spread"[N] (int64) and
        "spread_chain"[N]: the largest D(r, n) and the lowest chain that has it ((0, 0, -1)
        without a pooled chain); "chain_dist"[R] (int64): the sum of the chain's D;
        "chain_agree"[R]: the sequences whose chain mode is the pool's ((-1, -1) for a chain
        that is not pooled); "n_pooled"[1].  A chain is pooled when its sequence 0 has n_counted
        counts (the summaries' rule) or, with pooled[R] given, when its entry is non-zero
        (ListChainStats.finished() for list chains, whose rows do not sum to n_counted)."""
        occ = np.ascontiguousarray(occupancy, dtype=np.int32)
        H = int(self.lib.gs_occupancy_size(self.h, int(W)))
        if occ.ndim != 2 or (H >= 0 and occ.shape[1] != H):
            raise ArgumentError(GS_E_ARG, "occupancy needs the shape [chains, bins]")
        R = occ.shape[0]
        mask = None
        if pooled is not None:
            mask = np.ascontiguousarray(np.asarray(pooled) != 0, dtype=np.int32)
            if mask.shape != (R,):
                raise ArgumentError(GS_E_ARG, "pooled needs one entry per chain")
        out = self._agreement_outputs(R)
        self._check(self.lib.gs_occupancy_agreement(
            self.h, int(W), _ptr(occ) if R > 0 else None, R, int(n_counted),
            _ptr(mask) if R > 0 else None, *(_ptr(out[k]) for k in self._AGREEMENT)))
        out["n_pooled"] = out.pop("agree_n_pooled")
        return out

    def motif_run_batch_agreement(self, W: int, pc: float, cutoff: float, n_sweeps: int, seeds,
                                  pos=None, init_mode: int = 0, first_sweep: int = 0, u=None,
                                  burn_in: int = 0, thin: int = 1, occupancy: bool = False,
                                  ic: bool = True, best: bool = True, modes: bool = True,
                                  counts: bool = True, pool: bool = True, agreement: bool = True,
                                  strict: bool = False):
        """motif_run_batch_summary with the chains' agreement with their pool reduced on the
        device behind the summary (gs_motif_run_batch_agreement) -> (pos[R, N], pwms[R, N],
        status[R], stats), stats with the arrays of occupancy_agreement ("agree", "spread",
        "spread_chain", "chain_agree", "chain_dist", and the pool's count as "agree_n_pooled")
        besides those of motif_run_batch_summary.  A chain that raised is not pooled.  The bins
        are downloaded only with occupancy=True; agreement=False is motif_run_batch_summary."""
        seeds, pos, init_mode, u = self._run_batch_args(n_sweeps, seeds, pos, init_mode, u)
        R, T = len(seeds), int(n_sweeps)
        burn_in, thin = int(burn_in), int(thin)
        n_counted = self._n_counted(burn_in, thin, T)
        pwms = np.zeros((R, self.n_local), np.float64)
        status = np.zeros(R, np.int32)
        H = int(self.lib.gs_occupancy_size(self.h, int(W)))
        stats = self._stats_outputs(W, (R,), n_counted, occupancy, ic, best, H=H)
        stats.update(self._summary_outputs(W if H >= 0 else None, R, modes, counts, pool))
        if agreement:
            stats.update(self._agreement_outputs(R))
        st = self.lib.gs_motif_run_batch_agreement(
            self.h, int(W), float(pc), float(cutoff), T, _ptr(seeds), R, int(first_sweep),
            int(init_mode), _ptr(u), burn_in, thin, _ptr(pos), _ptr(pwms), _ptr(status),
            _ptr(stats.get("occupancy")), _ptr(stats.get("ic")), _ptr(stats.get("best_sweep")),
            _ptr(stats.get("best_pos")), _ptr(stats.get("best_pwms")),
            _ptr(stats.get("mode_pos")), _ptr(stats.get("mode_count")), _ptr(stats.get("counts")),
            _ptr(stats.get("pooled_pos")), _ptr(stats.get("pooled_count")),
            _ptr(stats.get("pooled_counts")), _ptr(stats.get("n_pooled")),
            *(_ptr(stats.get(k)) for k in self._AGREEMENT))
        if st != GS_OK and (strict or not status.any()):
            self._check(st)
        stats["n_counted"] = n_counted
        return pos, pwms, status, stats

    def agreement_last_ms(self) -> float:
        """Device milliseconds of the last chain agreement's reduction."""
        out = np.zeros(1, np.float64)
        self._check(self.lib.gs_agreement_last_ms(self.h, _ptr(out)))
        return float(out[0])

    def _run_multi_batch_args(self, motif_amount, n_sweeps, seeds, cnt, pos, init_mode, cap, u):
        """The chains' seeds, lists and uniforms as the library takes them (motif_run_multi_batch
        and motif_run_multi_batch_stats) -> (seeds, cnt, pos, init_mode, cap, u)."""
        cap = int(cap or motif_amount)
        seeds = np.array([int(s) & (2**64 - 1) for s in seeds], dtype=np.uint64)
        R = len(seeds)
        if (cnt is None) != (pos is None):
            raise ArgumentError(GS_E_ARG, "cnt and pos go together")
        if cnt is not None:
            init_mode = -1
            cnt = np.array(cnt, dtype=np.int32, copy=True)
            pos = np.array(pos, dtype=np.int32, copy=True)
            if cnt.shape != (R, self.n_local) or pos.size != R * self.n_local * max(cap, 0):
                raise ArgumentError(GS_E_ARG, "cnt / pos need one row per seed, one list per sequence")
            pos = np.ascontiguousarray(pos.reshape(R, self.n_local, cap))
        else:
            if init_mode not in (0, 1):
                raise ArgumentError(GS_E_ARG, "init_mode must be 0 or 1 when no starts are given")
            cnt = np.zeros((R, self.n_local), np.int32)
            pos = np.full((R, self.n_local, max(cap, 0)), -1, np.int32)
        if u is not None:
            u = np.ascontiguousarray(u, dtype=np.float64)
            if u.shape != (R, max(int(n_sweeps), 0), self.n_local):
                raise ArgumentError(GS_E_ARG, "u needs the shape [chains, sweeps, sequences]")
        return seeds, cnt, pos, init_mode, cap, u

    def motif_run_multi_batch(self, motif_amount: int, W: int, pc: float, cutoff: float,
                              n_sweeps: int, seeds, cnt=None, pos=None, init_mode: int = 0,
                              first_sweep: int = 0, cap: int | None = None, u=None,
                              strict: bool = False):
        """R independent chains of n_sweeps sweeps with Positions lists (any motifAmount) in
        one call, row r exactly n_sweeps motif_sweep_multi calls, each fed the previous
        output, with the counter RNG's uniforms of seeds[r] -> (cnt[R, N], pos[R, N, cap],
        pwms[R, N], status[R]).  The starts are the lists (cnt[R, N], pos[R, N, cap]; implies
        init_mode -1) or those of random_starts(W, pc, seeds[r], init_mode) as one-position
        lists.  u[R, n_sweeps, N] replaces the uniforms.  pwms is unspecified for n_sweeps =
        0.  A chain that raises (status[r] != 0) leaves the other rows valid; errors of the
        call itself raise, and with strict=True so does a chain's."""
        seeds, cnt, pos, init_mode, cap, u = self._run_multi_batch_args(
            motif_amount, n_sweeps, seeds, cnt, pos, init_mode, cap, u)
        R = len(seeds)
        pwms = np.zeros((R, self.n_local), np.float64)
        status = np.zeros(R, np.int32)
        st = self.lib.gs_motif_run_multi_batch(
            self.h, int(motif_amount), int(W), float(pc), float(cutoff), int(n_sweeps), _ptr(seeds),
            R, int(first_sweep), int(init_mode), cap, _ptr(u), _ptr(cnt), _ptr(pos), _ptr(pwms),
            _ptr(status))
        if st != GS_OK and (strict or not status.any()):
            self._check(st)
        return cnt, pos, pwms, status

    def motif_run_multi_batch_stats(self, motif_amount: int, W: int, pc: float, cutoff: float,
                                    n_sweeps: int, seeds, cnt=None, pos=None, init_mode: int = 0,
                                    first_sweep: int = 0, cap: int | None = None, u=None,
                                    burn_in: int = 0, thin: int = 1, occupancy: bool = True,
                                    sites: bool = True, ic: bool = True, best: bool = True,
                                    strict: bool = False):
        """motif_run_multi_batch with statistics of the chains' sweeps, gathered on the device
        with no host wait between sweeps -> (cnt[R, N], pos[R, N, cap], pwms[R, N], status[R],
        stats).  Sweep t counts when t >= burn_in and (t - burn_in) % thin == 0.  stats is a
        dict of the parts asked for: "occupancy"[R, H] with "offsets"[N + 1] (bin off[n]: the
        counted sweeps whose list of sequence n is empty, bin off[n] + 1 + k: those whose list
        contains start k); "sites"[R, N, motif_amount + 1] (the counted sweeps whose list of
        sequence n has that length); "ic"[R, n_counted], the sum of the PWMS of each counted
        sweep in the fixed order of sampler.informationContent; "best_sweep"[R] (first_sweep +
        t of the first largest ic, -1: none), "best_cnt"[R, N], "best_pos"[R, N, cap] and
        "best_pwms"[R, N].  A chain that raises in sweep t contributes nothing from t on (its
        ic entries are NaN).  With no part asked for this is motif_run_multi_batch."""
        seeds, cnt, pos, init_mode, cap, u = self._run_multi_batch_args(
            motif_amount, n_sweeps, seeds, cnt, pos, init_mode, cap, u)
        R, T, M = len(seeds), int(n_sweeps), int(motif_amount)
        burn_in, thin = int(burn_in), int(thin)
        pwms = np.zeros((R, self.n_local), np.float64)
        status = np.zeros(R, np.int32)
        stats = self._stats_outputs(W, (R,), self._n_counted(burn_in, thin, T), occupancy, ic, best,
                                    sites, M, cap)
        st = self.lib.gs_motif_run_multi_batch_stats(
            self.h, M, int(W), float(pc), float(cutoff), T, _ptr(seeds), R, int(first_sweep),
            int(init_mode), cap, _ptr(u), burn_in, thin, _ptr(cnt), _ptr(pos), _ptr(pwms),
            _ptr(status), _ptr(stats.get("occupancy")), _ptr(stats.get("sites")),
            _ptr(stats.get("ic")), _ptr(stats.get("best_sweep")), _ptr(stats.get("best_cnt")),
            _ptr(stats.get("best_pos")), _ptr(stats.get("best_pwms")))
        if st != GS_OK and (strict or not status.any()):
            self._check(st)
        return cnt, pos, pwms, status, stats

    _LIST_SUMMARY_KEYS = ("mode_sites", "mode_sites_count", "mode_cnt", "mode_pos", "mode_count",
                          "counts", "pooled_sites", "pooled_sites_count", "pooled_cnt",
                          "pooled_pos", "pooled_count", "pooled_counts", "n_pooled")

    def _list_summary_outputs(self, W, M, R, modes, counts, pool):
        """The output arrays of a list chain summary of R chains -> dict (the library's order:
        _LIST_SUMMARY_KEYS)."""
        cells = self._summary_cells(W)
        N, M = self.n_local, max(int(M), 0)
        out = {}
        if modes:
            out["mode_sites"] = np.zeros((R, N), np.int32)
            out["mode_sites_count"] = np.zeros((R, N), np.int32)
            out["mode_cnt"] = np.zeros((R, N), np.int32)
            out["mode_pos"] = np.full((R, N, M), -1, np.int32)
            out["mode_count"] = np.zeros((R, N, M), np.int32)
        if counts:
            out["counts"] = np.zeros((R, max(cells, 0)), np.int64)
        if pool:
            out["pooled_sites"] = np.zeros(N, np.int32)
            out["pooled_sites_count"] = np.zeros(N, np.int64)
            out["pooled_cnt"] = np.zeros(N, np.int32)
            out["pooled_pos"] = np.full((N, M), -1, np.int32)
            out["pooled_count"] = np.zeros((N, M), np.int64)
            out["pooled_counts"] = np.zeros(max(cells, 0), np.int64)
            out["n_pooled"] = np.zeros(1, np.int32)
        return out

    def list_occupancy_summary(self, W: int, motif_amount: int, occupancy, sites, n_counted: int,
                               modes: bool = True, counts: bool = True,
                               pool: bool = True) -> dict:
        """The reduction of caller-held list histograms occupancy[R, H] and site counts
        sites[R, N, motif_amount + 1] (a motif_run_multi_batch_stats call's, or the sums of
        several) on the device (gs_list_occupancy_summary) -> dict of the groups asked for.
        Per chain: "mode_sites"[R, N], the first most frequent site count c of every sequence,
        with "mode_sites_count"[R, N]; "mode_cnt"[R, N], "mode_pos"[R, N, M] and
        "mode_count"[R, N, M]: the c most occupied starts pairwise more than W apart, taken
        greedily (the first among equals), ascending, -1 / 0 past mode_cnt; "counts"[R, A W +
        A], the count matrix summed over the counted states in counts()' layout.  Pooled over
        the chains every sequence of which has n_counted site counts: "pooled_sites"[N],
        "pooled_sites_count"[N] (int64), "pooled_cnt"[N], "pooled_pos"[N, M],
        "pooled_count"[N, M] (int64), "pooled_counts"[A W + A] and "n_pooled"[1]."""
        occ = np.ascontiguousarray(occupancy, dtype=np.int32)
        sites = np.ascontiguousarray(sites, dtype=np.int32)
        H, M = int(self.lib.gs_occupancy_size(self.h, int(W))), int(motif_amount)
        if occ.ndim != 2 or (H >= 0 and occ.shape[1] != H):
            raise ArgumentError(GS_E_ARG, "occupancy needs the shape [chains, bins]")
        R = occ.shape[0]
        if 1 <= M <= 16 and sites.shape != (R, self.n_local, M + 1):
            raise ArgumentError(GS_E_ARG,
                                "sites needs the shape [chains, sequences, motif_amount + 1]")
        out = self._list_summary_outputs(W if H >= 0 else None, M, R, modes, counts, pool)
        self._check(self.lib.gs_list_occupancy_summary(
            self.h, int(W), M, _ptr(occ) if R > 0 else None, _ptr(sites) if R > 0 else None, R,
            int(n_counted), *(_ptr(out.get(k)) for k in self._LIST_SUMMARY_KEYS)))
        return out

    def motif_run_multi_batch_summary(self, motif_amount: int, W: int, pc: float, cutoff: float,
                                      n_sweeps: int, seeds, cnt=None, pos=None,
                                      init_mode: int = 0, first_sweep: int = 0,
                                      cap: int | None = None, u=None, burn_in: int = 0,
                                      thin: int = 1, occupancy: bool = False,
                                      sites: bool = False, ic: bool = True, best: bool = True,
                                      modes: bool = True, counts: bool = True, pool: bool = True,
                                      strict: bool = False):
        """motif_run_multi_batch_stats with the chains' list summaries and the pooled one
        reduced on the device (gs_motif_run_multi_batch_summary) -> (cnt[R, N], pos[R, N, cap],
        pwms[R, N], status[R], stats), stats with the groups of list_occupancy_summary besides
        those of motif_run_multi_batch_stats and "n_counted".  The bins and the site counts are
        downloaded only with occupancy=True / sites=True."""
        seeds, cnt, pos, init_mode, cap, u = self._run_multi_batch_args(
            motif_amount, n_sweeps, seeds, cnt, pos, init_mode, cap, u)
        R, T, M = len(seeds), int(n_sweeps), int(motif_amount)
        burn_in, thin = int(burn_in), int(thin)
        n_counted = self._n_counted(burn_in, thin, T)
        pwms = np.zeros((R, self.n_local), np.float64)
        status = np.zeros(R, np.int32)
        H = int(self.lib.gs_occupancy_size(self.h, int(W)))
        stats = self._stats_outputs(W, (R,), n_counted, occupancy, ic, best, sites, M, cap, H)
        stats.update(self._list_summary_outputs(W if H >= 0 else None, M, R, modes, counts, pool))
        st = self.lib.gs_motif_run_multi_batch_summary(
            self.h, M, int(W), float(pc), float(cutoff), T, _ptr(seeds), R, int(first_sweep),
            int(init_mode), cap, _ptr(u), burn_in, thin, _ptr(cnt), _ptr(pos), _ptr(pwms),
            _ptr(status), _ptr(stats.get("occupancy")), _ptr(stats.get("sites")),
            _ptr(stats.get("ic")), _ptr(stats.get("best_sweep")), _ptr(stats.get("best_cnt")),
            _ptr(stats.get("best_pos")), _ptr(stats.get("best_pwms")),
            *(_ptr(stats.get(k)) for k in self._LIST_SUMMARY_KEYS))
        if st != GS_OK and (strict or not status.any()):
            self._check(st)
        stats["n_counted"] = n_counted
        return cnt, pos, pwms, status, stats

    def motif_run_multi(self, motif_amount: int, W: int, pc: float, cutoff: float, n_sweeps: int,
                        seed: int, cnt, pos, first_sweep: int = 0, cap: int | None = None):
        """n_sweeps chained sweeps with Positions lists on the device from (cnt, pos) ->
        (cnt, pos[N, cap], pwms): motif_run_multi_batch with one chain."""
        cap = int(cap or motif_amount)
        cnt, pos = self._lists(cnt, pos, cap)
        pwms = np.zeros(self.n_local, np.float64)
        self._check(self.lib.gs_motif_run_multi(self.h, int(motif_amount), int(W), float(pc),
                                                float(cutoff), int(n_sweeps),
                                                int(seed) & (2**64 - 1), int(first_sweep), cap,
                                                _ptr(cnt), _ptr(pos), _ptr(pwms)))
        return cnt, pos, pwms

    def run_multi_batch_last_ms(self):
        """Device milliseconds of the last motif_run_multi_batch or
        motif_run_multi_batch_stats: (starts and their aggregates, sweeps with the statistics
        launches)."""
        out = np.zeros(2, np.float64)
        self._check(self.lib.gs_run_multi_batch_last_ms(self.h, _ptr(out)))
        return float(out[0]), float(out[1])

    def run_multi_batch_last_info(self) -> dict:
        """Overflow handling of the last motif_run_multi_batch(_stats): pairs rescored by overflow
        launches, chains parked, resume rounds, the first arena's capacity."""
        out = np.zeros(4, np.int32)
        self._check(self.lib.gs_run_multi_batch_last_info(self.h, _ptr(out)))
        return dict(zip(("rescored", "parked", "resume_rounds", "arena"), (int(v) for v in out)))

    def set_fixed_pcv(self, pcv49) -> None:
        """The caller's ProbabilityCompositeVector (49 slots) for the ByPCV / WithBPV
        twins of every entry point; None clears it."""
        if pcv49 is None:
            self._check(self.lib.gs_set_fixed_pcv(self.h, None))
            return
        v = np.ascontiguousarray(pcv49, np.float64)
        if v.shape != (49,):
            raise ArgumentError(GS_E_ARG, "pcv needs the 49 CompositeVector slots")
        self._check(self.lib.gs_set_fixed_pcv(self.h, _ptr(v)))

    def set_fixed_ppm(self, ppm49, W: int | None = None) -> None:
        """The caller's PositionProbabilityMatrix (49 slot rows x W) for the
        initialiser (getMotifsWithBestPWMSOfPPM); None clears it."""
        if ppm49 is None:
            self._check(self.lib.gs_set_fixed_ppm(self.h, None, 0))
            return
        m = np.ascontiguousarray(ppm49, np.float64)
        if m.ndim != 2 or m.shape[0] != 49 or (W is not None and m.shape[1] != W):
            raise ArgumentError(GS_E_ARG, "ppm needs 49 slot rows x motifLength columns")
        self._check(self.lib.gs_set_fixed_ppm(self.h, _ptr(m), int(m.shape[1])))

    def site_scan(self, W: int, pc: float, pos):
        """getBestPWMSs of every target with the others at pos -> (score, pos)."""
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        if pos.shape != (self.n_local,):
            raise ArgumentError(GS_E_ARG, "pos needs one entry per sequence")
        score = np.empty(self.n_local, np.float64)
        out = np.empty(self.n_local, np.int32)
        self._check(self.lib.gs_site_scan(self.h, int(W), float(pc), _ptr(pos), _ptr(score),
                                          _ptr(out)))
        return score, out

    def site_refine(self, W: int, pc: float, shift: int, pos, score, max_passes: int = 1000):
        """shift 0 / -1 / +1: getBestPWMSsWithStartPositions / getLeftShiftedBestPWMSs /
        getRightShiftedBestPWMSs -> (pos, score, passes)."""
        pos = np.array(pos, dtype=np.int32, copy=True)
        score = np.array(score, dtype=np.float64, copy=True)
        if pos.shape != (self.n_local,) or score.shape != (self.n_local,):
            raise ArgumentError(GS_E_ARG, "pos and score need one entry per sequence")
        passes = C.c_int32(0)
        self._check(self.lib.gs_site_refine(self.h, int(W), float(pc), int(shift),
                                            int(max_passes), _ptr(pos), _ptr(score),
                                            C.byref(passes)))
        return pos, score, passes.value

    def site_sampling(self, W: int, pc: float, seed: int, init_mode: int = 0,
                      max_passes: int = 1000):
        """doSiteSampling (.fs:697-701) -> (pos, score, passes of the three stages)."""
        pos = np.empty(self.n_local, np.int32)
        score = np.empty(self.n_local, np.float64)
        passes = np.zeros(3, np.int32)
        self._check(self.lib.gs_site_sampling(self.h, int(W), float(pc), int(seed) & (2**64 - 1),
                                              int(init_mode), int(max_passes), _ptr(pos),
                                              _ptr(score), _ptr(passes)))
        return pos, score, passes

    def site_sampling_batch(self, W: int, pc: float, seeds, init_mode: int = 0,
                            max_passes: int = 1000, *, pcv=None, ppm=None):
        """R independent doSiteSampling runs in one call, row r exactly
        site_sampling(W, pc, seeds[r], ...): the chains' Gauss–Seidel passes run as R
        concurrent workgroups, their shifted passes side by side ->
        (pos[R, N], score[R, N], passes[R, 3], status[R]).  A chain that raises
        (status[r] != 0, e.g. GS_E_OVERFLOW) leaves the other rows valid; errors of the
        call itself raise.  pcv (49 slots) / ppm (49 x W): the WithBPV / WithPPM twins
        (gs_site_sampling_batch_fixed), row r what site_sampling gives on a context with
        set_fixed_pcv(pcv) / set_fixed_ppm(ppm)."""
        pcv, ppm = fixed_args(pcv, ppm, W)
        seeds = np.array([int(s) & (2**64 - 1) for s in seeds], dtype=np.uint64)
        R = len(seeds)
        pos = np.empty((R, self.n_local), np.int32)
        score = np.empty((R, self.n_local), np.float64)
        passes = np.zeros((R, 3), np.int32)
        status = np.zeros(R, np.int32)
        if pcv is None and ppm is None:
            st = self.lib.gs_site_sampling_batch(self.h, int(W), float(pc), _ptr(seeds), R,
                                                 int(init_mode), int(max_passes), _ptr(pos),
                                                 _ptr(score), _ptr(passes), _ptr(status))
        else:
            st = self.lib.gs_site_sampling_batch_fixed(
                self.h, int(W), float(pc), _ptr(pcv), _ptr(ppm), _ptr(seeds), R, int(init_mode),
                int(max_passes), _ptr(pos), _ptr(score), _ptr(passes), _ptr(status))
        if st != GS_OK and not status.any():
            self._check(st)
        return pos, score, passes, status

    def site_batch_last_ms(self):
        """Device milliseconds of the last site_sampling_batch: (starts, Gauss–Seidel
        launch, shifted passes)."""
        out = np.zeros(3, np.float64)
        self._check(self.lib.gs_site_batch_last_ms(self.h, _ptr(out)))
        return float(out[0]), float(out[1]), float(out[2])

    def counts(self, W: int, pos, A: int):
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        Cm = np.empty(A * W, np.int64)
        T = np.empty(A, np.int64)
        self._check(self.lib.gs_counts(self.h, int(W), _ptr(pos), _ptr(Cm), _ptr(T)))
        return Cm.reshape(A, W), T

    def random_starts(self, W: int, pc: float, seed: int, mode: int = 0):
        score = np.empty(self.n_local, np.float64)
        pos = np.empty(self.n_local, np.int32)
        self._check(self.lib.gs_random_starts(self.h, int(W), float(pc), int(seed) & (2**64 - 1),
                                              int(mode), _ptr(score), _ptr(pos)))
        return score, pos

    def random_starts_batch(self, W: int, pc: float, seeds, mode: int = 0):
        """R independent getPWMOfRandomStarts runs in one call, row r exactly
        random_starts(W, pc, seeds[r], mode): every chain in the same launches over the
        (chain, target) pairs -> (score[R, N], pos[R, N], status[R]).  It follows
        set_fixed_pcv / set_fixed_ppm as random_starts does.  A chain that raises
        (status[r] != 0, GS_E_OVERFLOW) leaves the other rows valid; errors of the call
        itself raise."""
        seeds = np.array([int(s) & (2**64 - 1) for s in seeds], dtype=np.uint64)
        R = len(seeds)
        score = np.zeros((R, self.n_local), np.float64)
        pos = np.zeros((R, self.n_local), np.int32)
        status = np.zeros(R, np.int32)
        st = self.lib.gs_random_starts_batch(self.h, int(W), float(pc), _ptr(seeds), R, int(mode),
                                             _ptr(score), _ptr(pos), _ptr(status))
        if st != GS_OK and not status.any():
            self._check(st)
        return score, pos, status

    def starts_batch_last_ms(self):
        """Device milliseconds of the last random_starts_batch: (counts or aggregates,
        scans)."""
        out = np.zeros(2, np.float64)
        self._check(self.lib.gs_starts_batch_last_ms(self.h, _ptr(out)))
        return float(out[0]), float(out[1])

    # -- host-staged aggregate exchange
    def best_pwms(self, W: int, pc: float, target: int, fcv49, ppm49):
        """getBestPWMSs (.fs:462-479) of local sequence `target` against the caller's
        FrequencyCompositeVector fcv49 (49 int slots) and PPM ppm49 (49 x W)."""
        f = np.ascontiguousarray(fcv49, np.int32).reshape(-1)
        p = np.ascontiguousarray(ppm49, np.float64).reshape(-1)
        if f.size != 49 or p.size != 49 * W:
            raise ArgumentError(GS_E_ARG, "fcv49 needs 49 slots, ppm49 49 x W")
        sc, pos = C.c_double(), C.c_int32()
        self._check(self.lib.gs_best_pwms(self.h, int(W), float(pc), int(target), _ptr(f),
                                          _ptr(p), C.byref(sc), C.byref(pos)))
        return sc.value, pos.value

    def agg_download(self) -> np.ndarray:
        n = int(self.lib.gs_agg_size(self.h))
        out = np.empty(n, np.int64)
        self._check(self.lib.gs_agg_download(self.h, _ptr(out)))
        return out

    def agg_upload(self, agg: np.ndarray) -> None:
        agg = np.ascontiguousarray(agg, np.int64)
        if agg.size != int(self.lib.gs_agg_size(self.h)):
            raise ArgumentError(GS_E_ARG, "aggregate buffer size mismatch")
        self._check(self.lib.gs_agg_upload(self.h, _ptr(agg)))

    # -- in-kernel exchange of the aggregate vector (include/gibbs_hip.h gs_exchange_*)
    def exchange_handle(self) -> bytes:
        """This context's exchange buffer as an IPC handle (64 bytes) for the other ranks."""
        buf = (C.c_uint8 * IPC_HANDLE_BYTES)()
        self._check(self.lib.gs_exchange_handle(self.h, buf))
        return bytes(buf)

    def exchange_open(self, handles: list[bytes], rank: int) -> None:
        """Map every rank's buffer (handles in rank order): the live and long sweeps then
        sum the ranks' aggregate partials in-kernel (no all-reduce after them)."""
        blob = b"".join(handles)
        if len(blob) != IPC_HANDLE_BYTES * len(handles):
            raise ArgumentError(GS_E_ARG, "IPC handles are 64 bytes each")
        arr = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        self._check(self.lib.gs_exchange_open(self.h, arr, len(handles), int(rank)))
        self._xch_open = True

    def exchange_close(self) -> None:
        self._xch_open = False
        self._check(self.lib.gs_exchange_close(self.h))

    def exchange_is_open(self) -> bool:
        return getattr(self, "_xch_open", False)

    # -- measurement
    def profile(self, enable: bool | int) -> None:
        """True: time every launch; k > 1: every k-th (sampling); False: off."""
        k = int(enable) if not isinstance(enable, bool) else (1 if enable else 0)
        self._check(self.lib.gs_profile_enable(self.h, k))

    def region_begin(self) -> None:
        self._check(self.lib.gs_profile_region_begin(self.h))

    def region_stop(self) -> None:
        """Record the region's stop event without waiting (region_end reads it)."""
        self._check(self.lib.gs_profile_region_stop(self.h))

    def region_end(self) -> float:
        """Device milliseconds since region_begin (synchronises)."""
        ms = C.c_double()
        self._check(self.lib.gs_profile_region_end(self.h, C.byref(ms)))
        return ms.value

    def profile_read(self):
        a, b, c, d = C.c_double(), C.c_int64(), C.c_double(), C.c_int64()
        self._check(self.lib.gs_profile_read(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value

    def sweep_kernel_name(self) -> str:
        """The kernel the next sweep of the current state runs (measurement records)."""
        return self.lib.gs_sweep_kernel_name(self.h).decode()

    def last_sweep_launch(self) -> dict:
        """The last gs_sweep_kernel launch: its EK (4 = the four-symbol kernel), lanes per
        sequence, wavefronts per workgroup, workgroups, and `one`: 1 when it took the
        four-symbol kernel's one-iteration path (include/gibbs_hip.h)."""
        v = np.zeros(4, np.int32)
        self._check(self.lib.gs_last_sweep_launch(self.h, _ptr(v)))
        out = dict(zip(("ek", "gl", "waves", "grid"), (int(x) for x in v)))
        # (an older build loaded by path for an A/B run has no such path)
        out["one"] = int(self.lib.gs_last_sweep_one(self.h)) if hasattr(self.lib, "gs_last_sweep_one") else 0
        return out

    def stats(self) -> dict:
        """Cumulative fallback counters (include/gibbs_hip.h gs_stats)."""
        v = np.zeros(len(STAT_NAMES), np.int64)
        self._check(self.lib.gs_stats(self.h, _ptr(v), len(v)))
        return dict(zip(STAT_NAMES, (int(x) for x in v)))

    def fallbacks(self) -> int:
        """Serial exact roulette picks taken so far."""
        return self.stats()["serial_picks"]

    def set_scan_mode(self, exact: bool) -> None:
        """exact=False: certified binary32 scan (default); True: binary64 for every window."""
        self._check(self.lib.gs_set_scan_mode(self.h, SCAN_EXACT if exact else SCAN_CERTIFIED))

    def fastmath_check(self) -> tuple[float, float]:
        """(max |log2 error|, max relative exp2 error) of the device transcendentals."""
        a, b = C.c_double(), C.c_double()
        self._check(self.lib.gs_fastmath_check(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value


def uniform(seed: int, stream: int, index: int) -> float:
    return float(load_library().gs_uniform(seed & (2**64 - 1), stream, index))


def stream_sweep(t: int) -> int:
    return (1 << 40) | int(t)
