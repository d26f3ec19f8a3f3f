"""somatic-sniper_amd -- MI355X-native SomaticSniper site scorer (Python host mirror).

The product is the C ABI in ``include/sniper_amd.h`` implemented by
``libsniper_amd.so`` (HIP kernels for gfx950 + host C).  This module is a thin
ctypes binding that mirrors the reference's interface for the scoring path:

=============================================  ===========================================
reference (src/lib/sniper/...)                 here
=============================================  ===========================================
``sniper_maqcns_init/prepare`` +               ``Context(params)`` (tables built on the
``qAddTableInit/makeSoloPrior/                 host, uploaded to the GPU)
make_joint_prior`` (main.c:115-127)
``sniper_maqcns_glfgen(n, pl, ref_base, bm)``  ``Context.sniper_maqcns_glfgen(reads, ref_char)``
(sniper_maqcns.c:127)
``sniper_glf2cns(g, q_r)`` (:250)               ``Context.sniper_glf2cns(...)`` (from the GPU
                                               consensus word)
``glf_somatic(tid,pos,n1,n2,pl1,pl2,d,fh)``    ``Context.glf_somatic(ref_char, reads_t, reads_n)``
(somatic_sniper.c:109)                         single site, same return value
``bam_sspileup_file`` driving the callback     ``Context.score_batch`` (host arrays) and
(sniper_pileup.c:226-266)                      ``Context.score_device`` (HBM-resident)
=============================================  ===========================================

There is no CPU fallback: if the shared library or a GPU is missing every entry
point raises.  (The CPU restatement under ``oracle/`` is test infrastructure and
is never imported from here.)
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

__all__ = [
    "Params", "Synth", "Batch", "Context", "SniperError", "library_path", "load_library",
    "synth_batch_host", "model_check", "pack_read", "SS_GLF_DTYPE", "SS_CALL_DTYPE", "EXPORTED_SYMBOLS",
    "Inflater", "bgzf_scan", "inflate_cpu",
    "Pileup", "PileupState", "PileupRegion", "pileup_plan", "pileup_region_cpu",
]

_HERE = os.path.dirname(os.path.abspath(__file__))

SS_OK, SS_E_INVAL, SS_E_HIP, SS_E_NOMEM, SS_E_TABLES, SS_E_CAPACITY, SS_E_NODEV = 0, -1, -2, -3, -4, -5, -6
SS_E_CORRUPT = -7
SS_INF_OK, SS_INF_E_STREAM, SS_INF_E_SIZE, SS_INF_E_CRC = 0, 1, 2, 3   # per-member inflate statuses

# every symbol include/sniper_amd.h declares
EXPORTED_SYMBOLS = (
    "ss_abi_version", "ss_strerror", "ss_params_default", "ss_ctx_create", "ss_ctx_destroy",
    "ss_score_batch_device", "ss_score_batch_host", "ss_ctx_check", "ss_table_hashes",
    "ss_table_copy", "ss_synth_default", "ss_synth_batch_host", "ss_synth_batch_device",
    "ss_set_kernel_timing", "ss_last_kernel_ms", "ss_kernel_time_log", "ss_kernel_time_log_k", "ss_model_check", "ss_model_pinned",
    "ss_model_last_source",
    "ss_host_alloc", "ss_host_free",
    "ss_inflate_create", "ss_inflate_destroy", "ss_inflate_members_device", "ss_inflate_members_host",
    "ss_inflate_members_cpu", "ss_inflate_check", "ss_bgzf_scan",
    "ss_pileup_create", "ss_pileup_destroy", "ss_pileup_check", "ss_pileup_plan", "ss_pileup_count_device",
    "ss_pileup_fill_device", "ss_pileup_region_host", "ss_pileup_region_cpu",
    "ss_pileup_plan_device", "ss_pileup_split_cpu", "ss_bam_header_scan",
)


class SniperError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        lib = _LIB
        msg = lib.ss_strerror(code).decode() if lib is not None else str(code)
        super().__init__(f"{what}: {msg} (code {code})" if what else f"{msg} (code {code})")
        self.code = code


# --------------------------------------------------------------------------- structs
class Params(C.Structure):
    """ss_params_t -- CLI options of bam-somaticsniper (main.c:70-99)."""
    _fields_ = [
        ("theta", C.c_float), ("n_hap", C.c_int), ("het_rate", C.c_float), ("eta", C.c_float),
        ("cap_mapQ", C.c_int), ("min_somatic_qual", C.c_int), ("use_priors", C.c_int),
        ("use_joint_priors", C.c_int), ("somatic_rate", C.c_double), ("include_loh", C.c_int),
        ("include_gor", C.c_int),
    ]

    @classmethod
    def default(cls, **kw) -> "Params":
        p = cls()
        load_library().ss_params_default(C.byref(p))
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        return p


class _Batch(C.Structure):
    _fields_ = [("n_sites", C.c_uint64), ("ref", C.c_void_p), ("off_tumor", C.c_void_p),
                ("off_normal", C.c_void_p), ("reads_tumor", C.c_void_p),
                ("reads_normal", C.c_void_p)]


class _Out(C.Structure):
    _fields_ = [("score", C.c_void_p), ("calls", C.c_void_p), ("calls_cap", C.c_uint32),
                ("n_calls", C.c_void_p), ("glf", C.c_void_p), ("n_qadd_clamped", C.c_void_p)]


class Synth(C.Structure):
    """ss_synth_t -- deterministic synthetic pileup model."""
    _fields_ = [
        ("seed", C.c_uint64), ("shard", C.c_uint32), ("lambda_tumor", C.c_double),
        ("lambda_normal", C.c_double), ("fixed_depth", C.c_int), ("p_error", C.c_double),
        ("p_nbase", C.c_double), ("p_eq", C.c_double), ("p_iupac", C.c_double),
        ("p_del", C.c_double), ("p_mapq60", C.c_double), ("baseq_lo", C.c_int),
        ("baseq_hi", C.c_int), ("mapq_hi", C.c_int), ("p_wild_qual", C.c_double),
        ("p_somatic", C.c_double), ("vaf", C.c_double), ("p_germline", C.c_double),
        ("p_ref_n", C.c_double), ("p_ref_lower", C.c_double), ("p_ref_iupac", C.c_double),
    ]

    @classmethod
    def default(cls, lambda_tumor: float, lambda_normal: float, **kw) -> "Synth":
        s = cls()
        load_library().ss_synth_default(C.byref(s), C.c_double(lambda_tumor), C.c_double(lambda_normal))
        for k, v in kw.items():
            if not hasattr(s, k):
                raise AttributeError(k)
            setattr(s, k, v)
        return s


SS_GLF_DTYPE = np.dtype([("ref_base", "u1"), ("max_mapQ", "u1"), ("lk", "u1", (10,)),
                         ("min_lk", "u1"), ("pad", "u1"), ("depth", "<u4")], align=True)
SS_CALL_DTYPE = np.dtype([("site", "<u4"), ("somatic_score", "<i4"), ("cns_tumor", "<u4"),
                          ("cns_normal", "<u4"), ("joint_cq", "<i2"), ("snp_q_tumor", "u1"),
                          ("snp_q_normal", "u1"), ("joint_gt_tumor", "u1"),
                          ("joint_gt_normal", "u1"), ("status_tumor", "u1"),
                          ("status_normal", "u1"), ("ref_base4", "u1"), ("flags", "u1"),
                          ("pad", "<u2")], align=True)
assert SS_GLF_DTYPE.itemsize == 20 and SS_CALL_DTYPE.itemsize == 28


def pack_read(mapq: int, baseq: int, nt16: int, strand: int) -> int:
    """SS_READ_PACK: mapQ[7:0] baseQ[15:8] nt16[19:16] strand[20]."""
    return (mapq & 0xFF) | (baseq & 0xFF) << 8 | (nt16 & 0xF) << 16 | (strand & 1) << 20


@dataclass
class Batch:
    """A CSR batch of pileup sites (host numpy arrays)."""
    ref: np.ndarray          # u8 [n]
    off_tumor: np.ndarray    # u32 [n+1]
    off_normal: np.ndarray   # u32 [n+1]
    reads_tumor: np.ndarray  # u32
    reads_normal: np.ndarray  # u32

    @property
    def n_sites(self) -> int:
        return int(self.ref.shape[0])

    def site(self, i: int):
        t = self.reads_tumor[self.off_tumor[i]:self.off_tumor[i + 1]]
        n = self.reads_normal[self.off_normal[i]:self.off_normal[i + 1]]
        return int(self.ref[i]), t, n

    @classmethod
    def from_sites(cls, sites) -> "Batch":
        """sites: iterable of (ref_char:int|str, tumor_reads, normal_reads)."""
        ref, ot, on, rt, rn = [], [0], [0], [], []
        for r, t, n in sites:
            ref.append(ord(r) if isinstance(r, str) else int(r))
            rt.extend(int(x) for x in t)
            rn.extend(int(x) for x in n)
            ot.append(len(rt))
            on.append(len(rn))
        return cls(np.asarray(ref, np.uint8), np.asarray(ot, np.uint32), np.asarray(on, np.uint32),
                   np.asarray(rt, np.uint32), np.asarray(rn, np.uint32))

    def contiguous(self) -> "Batch":
        return Batch(*(np.ascontiguousarray(a) for a in (self.ref, self.off_tumor, self.off_normal,
                                                            self.reads_tumor, self.reads_normal)))

    def pinned(self) -> "Batch":
        """A copy whose arrays live in page-locked memory from ss_host_alloc
        (ss_score_batch_host then copies them to the device without staging).
        The memory is freed when the returned arrays are garbage-collected."""
        import weakref
        lib = load_library()
        out = []
        for a in (self.ref, self.off_tumor, self.off_normal, self.reads_tumor, self.reads_normal):
            nbytes = max(1, a.nbytes)
            p = lib.ss_host_alloc(nbytes)
            if not p:
                raise MemoryError("ss_host_alloc failed")
            buf = (C.c_char * nbytes).from_address(p)
            v = np.frombuffer(buf, dtype=a.dtype, count=a.size)
            v[...] = a
            weakref.finalize(buf, lib.ss_host_free, p)
            out.append(v)
        return Batch(*out)

    def algorithmic_bytes(self) -> int:
        """4 B per packed read + 16 B per site."""
        return 4 * (int(self.off_tumor[-1]) + int(self.off_normal[-1])) + 16 * self.n_sites


# --------------------------------------------------------------------------- library
_LIB = None


def library_path() -> str:
    return os.environ.get("SNIPER_AMD_LIB") or os.path.join(_HERE, "libsniper_amd.so")


def load_library():
    """Load libsniper_amd.so; raise loudly if it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(f"libsniper_amd.so not found at {path}: run __graft_entry__.build() "
                           f"(make -C somatic-sniper_amd); there is no CPU fallback")
    if os.environ.get("SNIPER_AMD_NO_TORCH") != "1":
        # One HIP runtime per process: PyTorch ships its own libamdhip64 with the
        # same soname (libamdhip64.so.7).  Loading torch first makes our NEEDED
        # entry bind to torch's copy, so device pointers and streams handed over
        # from torch tensors live in the same runtime as our kernels.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = C.CDLL(path)
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    lib.ss_abi_version.restype = C.c_int
    lib.ss_strerror.restype = C.c_char_p
    lib.ss_strerror.argtypes = [C.c_int]
    lib.ss_params_default.argtypes = [vp]
    lib.ss_ctx_create.argtypes = [vp, C.c_int, C.POINTER(vp)]
    lib.ss_ctx_destroy.argtypes = [vp]
    lib.ss_score_batch_device.argtypes = [vp, vp, vp, vp]
    lib.ss_score_batch_host.argtypes = [vp, vp, vp]
    lib.ss_host_alloc.restype = vp
    lib.ss_host_alloc.argtypes = [C.c_size_t]
    lib.ss_host_free.argtypes = [vp]
    lib.ss_ctx_check.argtypes = [vp]
    lib.ss_table_hashes.argtypes = [vp, vp, vp, vp, vp]
    lib.ss_table_copy.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.ss_synth_default.argtypes = [vp, C.c_double, C.c_double]
    lib.ss_synth_batch_host.argtypes = [vp, u64, u64, vp, vp, vp, vp, vp, vp, vp]
    lib.ss_synth_batch_device.argtypes = [vp, vp, u64, u64, vp, vp, vp, vp, vp, vp, vp]
    lib.ss_set_kernel_timing.argtypes = [vp, C.c_int]
    lib.ss_last_kernel_ms.argtypes = [vp]
    lib.ss_last_kernel_ms.restype = C.c_double
    lib.ss_model_check.argtypes = [vp, vp, vp]
    lib.ss_model_pinned.argtypes = [vp]
    if hasattr(lib, "ss_model_last_source"):      # absent from round-1 builds (A/B runs against them)
        lib.ss_model_last_source.restype = C.c_int
    lib.ss_kernel_time_log.argtypes = [vp, vp, C.c_int]
    lib.ss_kernel_time_log_k.argtypes = [vp, C.c_int, vp, C.c_int]
    lib.ss_inflate_create.argtypes = [C.c_int, u32, C.POINTER(vp)]
    lib.ss_inflate_destroy.argtypes = [vp]
    lib.ss_inflate_destroy.restype = None
    lib.ss_inflate_check.argtypes = [vp]
    lib.ss_inflate_members_device.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp]
    lib.ss_inflate_members_host.argtypes = [vp, vp, vp, u32, vp, vp, vp]
    lib.ss_inflate_members_cpu.argtypes = [vp, vp, u32, vp, vp, vp]
    lib.ss_bgzf_scan.argtypes = [vp, C.c_size_t, vp, vp, u32, C.POINTER(u32), C.POINTER(C.c_size_t)]
    lib.ss_pileup_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.ss_pileup_destroy.argtypes = [vp]
    lib.ss_pileup_destroy.restype = None
    lib.ss_pileup_check.argtypes = [vp]
    lib.ss_pileup_plan.argtypes = [vp, C.c_size_t, C.c_int, C.c_int, vp, vp, vp, vp, u32, C.POINTER(u32),
                                   C.POINTER(C.c_size_t)]
    lib.ss_pileup_count_device.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_int32, C.c_int32, C.POINTER(u64),
                                           C.POINTER(u64), C.POINTER(u64), vp]
    lib.ss_pileup_fill_device.argtypes = [vp, vp, vp]
    lib.ss_pileup_region_host.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_int32, C.c_int32, vp]
    lib.ss_pileup_region_cpu.argtypes = [vp, vp, vp, C.c_int64, C.c_int32, C.c_int32, vp]
    lib.ss_pileup_plan_device.argtypes = [vp, vp, u64, C.c_int32, C.c_int, C.c_int, vp, vp, vp, vp, u32,
                                          C.POINTER(u32), C.POINTER(u64), vp, u32, C.POINTER(u32), C.POINTER(u32), vp]
    lib.ss_pileup_split_cpu.argtypes = [vp, u64, C.c_int32, u32, vp, u64, C.POINTER(u64), C.POINTER(u64),
                                        C.POINTER(C.c_int), C.POINTER(u32)]
    lib.ss_bam_header_scan.argtypes = [vp, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_size_t)]
    if hasattr(lib, "ss__test_poke_table"):         # test hook, not in the public header
        lib.ss__test_poke_table.argtypes = [vp, u64, C.c_int]
    if hasattr(lib, "ss__plan_phase_ms"):           # measurement hook, not in the public header
        lib.ss__plan_phase_ms.argtypes = [vp, C.POINTER(C.c_double)]
        lib.ss__plan_phase_ms.restype = None
    if hasattr(lib, "ss__test_route_counts"):       # test hook, not in the public header
        lib.ss__test_route_counts.argtypes = [vp, C.POINTER(C.c_uint32)]
    if lib.ss_abi_version() != 1:
        raise RuntimeError("libsniper_amd.so ABI mismatch")
    _LIB = lib
    return lib


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data if a.size else 0


def _check(rc: int, what: str):
    if rc != SS_OK:
        raise SniperError(rc, what)


def model_check(params: Params | None = None):
    """Build the model tables on the host (no GPU needed) and return their hashes and
    whether they equal a recorded run of the compiled reference (sniper_maqcns.c:27-100
    evaluated with this host's libm / x87, as the reference itself does)."""
    lib = load_library()
    p = params if params is not None else Params.default()
    h = (C.c_uint64 * 3)()
    qr = C.c_float()
    _check(lib.ss_model_check(C.byref(p), h, C.byref(qr)), "ss_model_check")
    return {"fk": f"{h[0]:016x}", "coef": f"{h[1]:016x}", "lhet": f"{h[2]:016x}", "q_r": qr.value,
            "pinned": bool(lib.ss_model_pinned(h)),
            "source": {0: "built", 1: "process", 2: "disk"}.get(
                lib.ss_model_last_source() if hasattr(lib, "ss_model_last_source") else -1, "none")}


def synth_batch_host(synth: Synth, first_site: int, n_sites: int) -> Batch:
    """Host twin of the device generator (bit-identical bytes)."""
    lib = load_library()
    ref = np.empty(n_sites, np.uint8)
    ot = np.empty(n_sites + 1, np.uint32)
    on = np.empty(n_sites + 1, np.uint32)
    nt, nn = C.c_uint64(), C.c_uint64()
    _check(lib.ss_synth_batch_host(C.byref(synth), first_site, n_sites, _ptr(ref), _ptr(ot), _ptr(on),
                                   None, None, C.byref(nt), C.byref(nn)), "ss_synth_batch_host")
    rt = np.empty(nt.value, np.uint32)
    rn = np.empty(nn.value, np.uint32)
    _check(lib.ss_synth_batch_host(C.byref(synth), first_site, n_sites, _ptr(ref), _ptr(ot), _ptr(on),
                                   _ptr(rt) or None, _ptr(rn) or None, C.byref(nt), C.byref(nn)),
           "ss_synth_batch_host")
    if nt.value == 0 or nn.value == 0:  # degenerate all-deleted batches
        rt = np.zeros(nt.value, np.uint32)
        rn = np.zeros(nn.value, np.uint32)
    return Batch(ref, ot, on, rt, rn)


class Context:
    """One scorer context on one GPU (sniper_maqcns_t + pu_data2_t equivalent)."""

    def __init__(self, params: Params | None = None, device: int = 0):
        self.lib = load_library()
        self.params = params if params is not None else Params.default()
        h = C.c_void_p()
        _check(self.lib.ss_ctx_create(C.byref(self.params), device, C.byref(h)), "ss_ctx_create")
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.ss_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- tables ------------------------------------------------------------------
    def table_hashes(self):
        fk, coef, lhet, qr = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_float()
        _check(self.lib.ss_table_hashes(self.h, C.byref(fk), C.byref(coef), C.byref(lhet),
                                        C.byref(qr)), "ss_table_hashes")
        return {"fk": f"{fk.value:016x}", "coef": f"{coef.value:016x}",
                "lhet": f"{lhet.value:016x}", "q_r": qr.value}

    # -- batches -----------------------------------------------------------------
    def score_batch(self, b: Batch, calls_cap: int | None = None, want_glf: bool = False):
        """Score a host batch; returns (score[n] i32, calls structured array, glf or None)."""
        b = b.contiguous()
        n = b.n_sites
        score = np.empty(n, np.int32)
        cap = max(16, n // 64) if calls_cap is None else calls_cap
        calls = np.zeros(cap, SS_CALL_DTYPE)
        glf = np.zeros((n, 2), SS_GLF_DTYPE) if want_glf else None
        ncalls, nclamp = C.c_uint32(), C.c_uint32()
        bt = _Batch(n, _ptr(b.ref), _ptr(b.off_tumor), _ptr(b.off_normal), _ptr(b.reads_tumor),
                    _ptr(b.reads_normal))
        out = _Out(_ptr(score), _ptr(calls), cap, C.addressof(ncalls),
                   _ptr(glf) if want_glf else None, C.addressof(nclamp))
        rc = self.lib.ss_score_batch_host(self.h, C.byref(bt), C.byref(out))
        if rc == SS_E_CAPACITY and ncalls.value > cap and calls_cap is None:
            return self.score_batch(b, calls_cap=int(ncalls.value), want_glf=want_glf)
        _check(rc, "ss_score_batch_host")
        self.last_clamped = int(nclamp.value)
        return score, calls[: min(ncalls.value, cap)].copy(), glf

    def score_device(self, ref, off_t, off_n, reads_t, reads_n, score, calls=None, calls_cap=0,
                     n_calls=None, glf=None, stream=None, n_sites=None):
        """Score an HBM-resident batch; arguments are torch CUDA tensors (or raw ints).
        Asynchronous on `stream` (torch.cuda.Stream or raw handle)."""
        def p(x):
            if x is None:
                return None
            return x if isinstance(x, int) else x.data_ptr()
        n = int(n_sites if n_sites is not None else ref.numel())
        bt = _Batch(n, p(ref), p(off_t), p(off_n), p(reads_t), p(reads_n))
        out = _Out(p(score), p(calls), calls_cap, p(n_calls), p(glf), None)
        sh = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
        _check(self.lib.ss_score_batch_device(self.h, C.byref(bt), C.byref(out), sh),
               "ss_score_batch_device")

    def synth_device(self, synth: Synth, first_site: int, n_sites: int, device=None):
        """Generate a synthetic batch directly in HBM; returns torch tensors."""
        import torch
        dev = device if device is not None else torch.device("cuda", self.device)
        ref = torch.empty(n_sites, dtype=torch.uint8, device=dev)
        ot = torch.empty(n_sites + 1, dtype=torch.int32, device=dev)
        on = torch.empty(n_sites + 1, dtype=torch.int32, device=dev)
        nt, nn = C.c_uint64(), C.c_uint64()
        torch.cuda.synchronize(dev)
        _check(self.lib.ss_synth_batch_device(self.h, C.byref(synth), first_site, n_sites,
                                              ref.data_ptr(), ot.data_ptr(), on.data_ptr(), None, None,
                                              C.byref(nt), C.byref(nn)), "ss_synth_batch_device")
        rt = torch.empty(max(1, nt.value), dtype=torch.int32, device=dev)
        rn = torch.empty(max(1, nn.value), dtype=torch.int32, device=dev)
        _check(self.lib.ss_synth_batch_device(self.h, C.byref(synth), first_site, n_sites,
                                              ref.data_ptr(), ot.data_ptr(), on.data_ptr(),
                                              rt.data_ptr(), rn.data_ptr(), C.byref(nt), C.byref(nn)),
               "ss_synth_batch_device")
        return {"ref": ref, "off_tumor": ot, "off_normal": on, "reads_tumor": rt,
                "reads_normal": rn, "n_reads": (int(nt.value), int(nn.value)), "n_sites": n_sites}

    def check(self):
        _check(self.lib.ss_ctx_check(self.h), "device work")

    def _poke_table(self, byte_offset: int, value: int):
        """Test hook: overwrite one byte of the device tables (ss_ctx_check must then fail)."""
        _check(self.lib.ss__test_poke_table(self.h, byte_offset, value), "ss__test_poke_table")

    def _route_counts(self):
        """Test hook: the latest launch's routing -- the deep triage's blocks,
        the sites left to the main kernel, those it queued for the group and
        the deep kernels."""
        out = (C.c_uint32 * 4)()
        _check(self.lib.ss__test_route_counts(self.h, out), "ss__test_route_counts")
        return {"deep_triage_blocks": out[0], "main_sites": out[1], "group_sites": out[2], "deep_sites": out[3]}

    def set_kernel_timing(self, enable: bool):
        _check(self.lib.ss_set_kernel_timing(self.h, 1 if enable else 0), "ss_set_kernel_timing")

    def last_kernel_ms(self) -> float:
        return float(self.lib.ss_last_kernel_ms(self.h))

    KERNELS = {"main": 0, "wide": 1, "deep": 2, "all": 3}   # SS_KT_*

    def kernel_time_log(self, kernel: str = "main") -> np.ndarray:
        """Durations (ms) of one kernel of every launch since set_kernel_timing(True):
        "main" (ss_score_main), "wide" (ss_score_group: the wide list), "deep" (ss_score_deep) or "all" (the launch)."""
        buf = np.zeros(4096, np.float64)
        n = self.lib.ss_kernel_time_log_k(self.h, self.KERNELS[kernel], buf.ctypes.data, buf.size)
        if n < 0:
            raise SniperError(n, "ss_kernel_time_log_k")
        return buf[:n].copy()

    # -- reference-named single-site helpers ---------------------------------------
    def glf_somatic(self, ref_char, reads_tumor, reads_normal) -> int:
        """Return value of glf_somatic (somatic_sniper.c:109) for one site, on the GPU."""
        s, _, _ = self.score_batch(Batch.from_sites([(ref_char, reads_tumor, reads_normal)]))
        return int(s[0])

    def sniper_maqcns_glfgen(self, reads, ref_char):
        """glf1_t of one sample (sniper_maqcns.c:127) computed by the GPU kernel."""
        _, _, g = self.score_batch(Batch.from_sites([(ref_char, reads, [pack_read(60, 30, 1, 0)])]),
                                   want_glf=True)
        return g[0, 0]

    @staticmethod
    def sniper_glf2cns_fields(cns: int):
        """Decode a consensus word: (cns, cns2, rms_mapQ, cnsQ, cnsQ2) (sniper_maqcns.h:28)."""
        return cns >> 28, (cns >> 24) & 0xF, (cns >> 16) & 0xFF, (cns >> 8) & 0xFF, cns & 0xFF


# --------------------------------------------------------------------------- BGZF inflation
def _u8(data) -> np.ndarray:
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, np.uint8)
    return np.frombuffer(bytes(data) if not isinstance(data, (bytes, bytearray, memoryview)) else data, np.uint8)


def bgzf_scan(data, cap: int | None = None):
    """Cut BGZF file bytes into members (ss_bgzf_scan).  Returns (comp_span, out_off,
    consumed): member i's DEFLATE data + trailer is data[comp_span[i, 0]:comp_span[i, 1]],
    its output data_out[out_off[i]:out_off[i + 1]]; `consumed` is where the first
    incomplete member (or the end of the data) starts."""
    lib = load_library()
    a = _u8(data)
    if cap is None:
        cap = a.size // 26 + 1                     # no member is shorter than header + 2 + trailer
    span = np.zeros((cap, 2), np.uint64)
    ooff = np.zeros(cap + 1, np.uint64)
    n, used = C.c_uint32(), C.c_size_t()
    _check(lib.ss_bgzf_scan(_ptr(a) or None, a.size, span.ctypes.data, ooff.ctypes.data, cap, C.byref(n),
                            C.byref(used)), "ss_bgzf_scan")
    return span[: n.value].copy(), ooff[: n.value + 1].copy(), int(used.value)


def _pack_members(data):
    """Members of BGZF file bytes, packed one after the other (the layout the
    inflate calls take): (comp, comp_off, out_off)."""
    a = _u8(data)
    span, ooff, used = bgzf_scan(a)
    if used != a.size:
        raise ValueError(f"incomplete BGZF member at byte {used} of {a.size}")
    lens = (span[:, 1] - span[:, 0]).astype(np.uint64)
    coff = np.zeros(len(span) + 1, np.uint64)
    np.cumsum(lens, out=coff[1:])
    comp = np.empty(int(coff[-1]), np.uint8)
    for i, (b, e) in enumerate(span):
        comp[int(coff[i]):int(coff[i + 1])] = a[int(b):int(e)]
    return comp, coff, ooff


def _member_args(comp, comp_off, out_off, out):
    comp = _u8(comp)
    comp_off = np.ascontiguousarray(comp_off, np.uint64)
    out_off = np.ascontiguousarray(out_off, np.uint64)
    n = len(comp_off) - 1
    if n < 0 or len(out_off) != n + 1:
        raise ValueError("comp_off and out_off must have n + 1 entries")
    if n and int(comp_off[-1]) > comp.size:
        raise ValueError("comp_off passes the end of comp")
    if out is None:
        out = np.zeros(int(out_off[-1]) if n else 0, np.uint8)
    elif n and int(out_off[-1]) > out.size:
        raise ValueError("out_off passes the end of out")
    return comp, comp_off, out_off, n, out, np.zeros(n, np.uint32)


def inflate_members_cpu(comp, comp_off, out_off, out=None):
    """ss_inflate_members_cpu: the shared decoder on the calling thread (no GPU)."""
    comp, comp_off, out_off, n, out, status = _member_args(comp, comp_off, out_off, out)
    _check(load_library().ss_inflate_members_cpu(_ptr(comp) or None, comp_off.ctypes.data, n, _ptr(out) or None,
                                                 out_off.ctypes.data, _ptr(status) or None),
           "ss_inflate_members_cpu")
    return out, status


def inflate_cpu(data):
    """Inflate BGZF file bytes with the shared decoder on the host:
    (bytes, status ndarray), as Inflater.inflate."""
    out, status = inflate_members_cpu(*_pack_members(data))
    return out.tobytes(), status


class Inflater:
    """BGZF members inflated on the GPU (ss_inflate_t): one wave per member."""

    def __init__(self, device: int = 0, max_members: int = 4096):
        self.lib = load_library()
        h = C.c_void_p()
        _check(self.lib.ss_inflate_create(device, max_members, C.byref(h)), "ss_inflate_create")
        self.h = h
        self.device = device
        self.max_members = max_members

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.ss_inflate_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def inflate_members(self, comp, comp_off, out_off, out=None):
        """Low-level call (ss_inflate_members_host): member i is
        comp[comp_off[i]:comp_off[i+1]] (DEFLATE data + 8-byte trailer), its output
        out[out_off[i]:out_off[i+1]].  Returns (out u8 ndarray, status u32 ndarray);
        more than max_members members go in several calls."""
        comp, comp_off, out_off, n, out, status = _member_args(comp, comp_off, out_off, out)
        for a in range(0, n, self.max_members):
            k = min(self.max_members, n - a)
            _check(self.lib.ss_inflate_members_host(self.h, _ptr(comp) or None, comp_off[a:].ctypes.data, k,
                                                    _ptr(out) or None, out_off[a:].ctypes.data,
                                                    status[a:].ctypes.data), "ss_inflate_members_host")
        return out, status

    def inflate_device(self, comp, comp_off, n, out, out_off, status, stream=None):
        """ss_inflate_members_device: torch CUDA tensors (or raw device addresses),
        asynchronous on `stream`."""
        def p(x):
            return x if isinstance(x, int) else x.data_ptr()
        sh = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
        _check(self.lib.ss_inflate_members_device(self.h, p(comp), p(comp_off), n, p(out), p(out_off), p(status),
                                                  sh), "ss_inflate_members_device")

    def inflate(self, data):
        """Scan BGZF file bytes, inflate every member on the GPU and return
        (bytes, status ndarray): the concatenated output (a failed member's bytes
        are zero) and one SS_INF_* status per member."""
        out, status = self.inflate_members(*_pack_members(data))
        return out.tobytes(), status

    def check(self):
        """Wait for the handle's stream; debug build: SS_E_CORRUPT if a guard band was overwritten."""
        _check(self.lib.ss_inflate_check(self.h), "ss_inflate_check")


# --------------------------------------------------------------------------- pileup from BAM records
SS_PILEUP_MAX_SPAN = 1 << 22
SS_PLAN_CHUNK = 16384                            # bytes per chunk of the device planner's walk
SS_BAM_MORE = 1                                  # bam_header_scan: the prefix ends inside the header
SS_PLAN_END_DATA, SS_PLAN_END_BLOCK = 1, 2       # why a record chain ended (pileup_split_cpu)
SS_RUN_DTYPE = np.dtype([("tid", "<i4"), ("first", "<u4"), ("n", "<u4"), ("lo", "<i4"), ("hi", "<i4")])   # ss_pileup_run_t


class PileupState(C.Structure):
    """ss_pileup_state_t -- the walk state pileup_plan carries from chunk to chunk."""
    _fields_ = [("has_prev", C.c_int32), ("tid", C.c_int32), ("w", C.c_int64), ("max_tid", C.c_int32),
                ("pad", C.c_int32)]


class _PileupSample(C.Structure):
    _fields_ = [("bytes", C.c_void_p), ("n_bytes", C.c_uint64), ("rec_off", C.c_void_p), ("from_", C.c_void_p),
                ("n", C.c_uint32), ("pad", C.c_uint32)]


class _PileupOut(C.Structure):
    _fields_ = [("cap_sites", C.c_uint64), ("cap_reads_t", C.c_uint64), ("cap_reads_n", C.c_uint64),
                ("pos", C.c_void_p), ("ref", C.c_void_p), ("raw_t", C.c_void_p), ("raw_n", C.c_void_p),
                ("off_t", C.c_void_p), ("off_n", C.c_void_p), ("reads_t", C.c_void_p), ("reads_n", C.c_void_p),
                ("n_sites", C.c_uint64), ("n_reads_t", C.c_uint64), ("n_reads_n", C.c_uint64),
                ("n_invalid", C.c_uint64)]


@dataclass
class PileupRegion:
    """The columns of one region: `batch` (what Context.score_batch takes) plus each
    site's position and raw depths.  rc is SS_OK, or SS_E_INVAL when n_invalid
    records failed validation (the other records' columns are all here)."""
    batch: Batch
    pos: np.ndarray          # i32 [n]
    raw_t: np.ndarray        # u32 [n]
    raw_n: np.ndarray        # u32 [n]
    rc: int = 0
    n_invalid: int = 0


def pileup_plan(data, mask: int = -1, thresh: int = 0, state: PileupState | None = None, cap: int | None = None):
    """ss_pileup_plan over uncompressed BAM record bytes (positioned after the
    header): (rec_off u64, from i32, tid i32, consumed).  `state` (a PileupState,
    updated in place) lets a file be planned in consecutive chunks; `cap` bounds
    the records kept by one call."""
    lib = load_library()
    a = _u8(data)
    if state is None:
        state = PileupState()
    if cap is None:
        cap = a.size // 36 + 1                     # no record is shorter than 36 bytes
    off = np.zeros(cap, np.uint64)
    frm = np.zeros(cap, np.int32)
    tid = np.zeros(cap, np.int32)
    n, used = C.c_uint32(), C.c_size_t()
    _check(lib.ss_pileup_plan(_ptr(a) or None, a.size, mask, thresh, C.byref(state), off.ctypes.data,
                              frm.ctypes.data, tid.ctypes.data, cap, C.byref(n), C.byref(used)), "ss_pileup_plan")
    k = n.value
    return off[:k].copy(), frm[:k].copy(), tid[:k].copy(), int(used.value)


def pileup_split_cpu(data, n_ref: int = 0, chunk: int = SS_PLAN_CHUNK, cap: int | None = None):
    """ss_pileup_split_cpu: the device planner's guess / walk / stitch / repair on the
    calling thread with chunks of `chunk` bytes.  Returns (rec_off u64 of every whole
    record of the chain, end_at, end_why (SS_PLAN_END_*), n_repaired)."""
    lib = load_library()
    a = _u8(data)
    if cap is None:
        cap = a.size // 36 + 1                     # no record is shorter than 36 bytes
    off = np.zeros(cap, np.uint64)
    n, end_at, why, rep = C.c_uint64(), C.c_uint64(), C.c_int(), C.c_uint32()
    _check(lib.ss_pileup_split_cpu(_ptr(a) or None, a.size, n_ref, chunk, _ptr(off) or None, cap, C.byref(n),
                                   C.byref(end_at), C.byref(why), C.byref(rep)), "ss_pileup_split_cpu")
    return off[: n.value].copy(), int(end_at.value), int(why.value), int(rep.value)


def bam_header_scan(data):
    """ss_bam_header_scan over a prefix of uncompressed BAM bytes: (n_ref, records_at),
    or None if the prefix ends inside the header."""
    lib = load_library()
    a = _u8(data)
    n_ref, at = C.c_int32(), C.c_size_t()
    rc = lib.ss_bam_header_scan(_ptr(a) or None, a.size, C.byref(n_ref), C.byref(at))
    if rc == SS_BAM_MORE:
        return None
    _check(rc, "ss_bam_header_scan")
    return int(n_ref.value), int(at.value)


def _pileup_sample(sample):
    """(bytes, rec_off, from) as numpy arrays -> (_PileupSample, arrays kept alive)."""
    data, off, frm = sample
    a = _u8(data)
    off = np.ascontiguousarray(off, np.uint64)
    frm = np.ascontiguousarray(frm, np.int32)
    if off.shape != frm.shape or off.ndim != 1:
        raise ValueError("rec_off and from must be 1-d arrays of one length")
    return _PileupSample(_ptr(a) or None, a.size, _ptr(off) or None, _ptr(frm) or None, off.size, 0), (a, off, frm)


def _pileup_region(call, what, tumor, normal, ref, lo, hi, caps, invalid_ok):
    st, keep_t = _pileup_sample(tumor)
    sn, keep_n = _pileup_sample(normal)
    r = None if ref is None else _u8(ref)
    ref_len = 0 if r is None else r.size
    out = _PileupOut()
    arrays = None
    for attempt in range(2):
        ns, nt, nn = caps if caps is not None else (0, 0, 0)
        arrays = (np.zeros(ns, np.int32), np.zeros(ns, np.uint8), np.zeros(ns, np.uint32), np.zeros(ns, np.uint32),
                  np.zeros(ns + 1, np.uint32), np.zeros(ns + 1, np.uint32), np.zeros(nt, np.uint32),
                  np.zeros(nn, np.uint32))
        out = _PileupOut(ns, nt, nn, *(a.ctypes.data for a in arrays))
        rc = call(C.byref(st), C.byref(sn), None if r is None else (_ptr(r) or None), ref_len, lo, hi, C.byref(out))
        if rc == SS_E_CAPACITY and caps is None and max(out.n_reads_t, out.n_reads_n) <= 0xC0000000:
            caps = (int(out.n_sites), int(out.n_reads_t), int(out.n_reads_n))      # the sizes needed
            continue
        break
    if rc != SS_OK and not (rc == SS_E_INVAL and invalid_ok and out.n_invalid):
        raise SniperError(rc, what)
    ns, nt, nn = int(out.n_sites), int(out.n_reads_t), int(out.n_reads_n)
    pos, refc, raw_t, raw_n, off_t, off_n, reads_t, reads_n = arrays
    return PileupRegion(Batch(refc[:ns], off_t[:ns + 1], off_n[:ns + 1], reads_t[:nt], reads_n[:nn]), pos[:ns],
                        raw_t[:ns], raw_n[:ns], rc, int(out.n_invalid))


def pileup_region_cpu(tumor, normal, ref, lo: int, hi: int, caps=None, invalid_ok: bool = False) -> PileupRegion:
    """ss_pileup_region_cpu: the columns of [lo, hi) built by the shared core on the
    calling thread (no GPU).  tumor / normal: (bytes, rec_off, from) of one contig's
    records in load order (pileup_plan); ref: the contig's bases (bytes / u8 array)
    or None.  caps: (sites, reads_t, reads_n) capacities (default: sized by a first
    call).  invalid_ok: return the columns (rc == SS_E_INVAL) when records failed
    validation instead of raising."""
    lib = load_library()
    return _pileup_region(lib.ss_pileup_region_cpu, "ss_pileup_region_cpu", tumor, normal, ref, lo, hi, caps,
                          invalid_ok)


class Pileup:
    """Pileup columns from BAM records on the GPU (ss_pileup_t)."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        h = C.c_void_p()
        _check(self.lib.ss_pileup_create(device, C.byref(h)), "ss_pileup_create")
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.lib.ss_pileup_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @staticmethod
    def _p(x):
        if x is None:
            return None
        return x if isinstance(x, int) else x.data_ptr()

    def count(self, tumor, normal, ref, ref_len: int, lo: int, hi: int, stream=None):
        """ss_pileup_count_device.  tumor / normal: (bytes, n_bytes, rec_off, from, n)
        of torch CUDA tensors or raw device addresses; ref: a tensor / address or
        None.  Synchronous; returns (n_sites, n_reads_t, n_reads_n)."""
        p = self._p
        smp = [_PileupSample(p(b), nb, p(o), p(f), n, 0) for b, nb, o, f, n in (tumor, normal)]
        ns, nt, nn = C.c_uint64(), C.c_uint64(), C.c_uint64()
        sh = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
        _check(self.lib.ss_pileup_count_device(self.h, C.byref(smp[0]), C.byref(smp[1]), p(ref), ref_len, lo, hi,
                                               C.byref(ns), C.byref(nt), C.byref(nn), sh), "ss_pileup_count_device")
        return int(ns.value), int(nt.value), int(nn.value)

    def fill(self, pos, ref, raw_t, raw_n, off_t, off_n, reads_t, reads_n, cap_sites: int, cap_reads_t: int,
             cap_reads_n: int, stream=None):
        """ss_pileup_fill_device into torch CUDA tensors (or raw device addresses),
        asynchronous on `stream`."""
        p = self._p
        out = _PileupOut(cap_sites, cap_reads_t, cap_reads_n, p(pos), p(ref), p(raw_t), p(raw_n), p(off_t), p(off_n),
                         p(reads_t), p(reads_n))
        sh = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
        _check(self.lib.ss_pileup_fill_device(self.h, C.byref(out), sh), "ss_pileup_fill_device")

    def region(self, tumor, normal, ref, lo: int, hi: int, caps=None, invalid_ok: bool = False) -> PileupRegion:
        """ss_pileup_region_host: numpy in, numpy out; arguments and result as
        pileup_region_cpu."""
        return _pileup_region(lambda *a: self.lib.ss_pileup_region_host(self.h, *a), "ss_pileup_region_host", tumor,
                              normal, ref, lo, hi, caps, invalid_ok)

    def region_device(self, tumor, normal, ref, lo: int, hi: int, stream=None):
        """Records (numpy, as for `region`) to the device, both passes there, and the
        batch stays in HBM: returns the dict of torch tensors Context.score_device
        takes (ref, off_tumor, off_normal, reads_tumor, reads_normal, n_sites) plus
        pos, raw_t, raw_n.  The fill is asynchronous on `stream`."""
        import torch
        dev = torch.device("cuda", self.device)
        smp = []
        for data, off, frm in (tumor, normal):
            a = _u8(data)
            off = np.ascontiguousarray(off, np.uint64)
            # only the bytes the records lie in: from the lowest offset to the end of the last block
            b0 = min(int(off.min()), a.size) if off.size else 0
            b1 = a.size
            last = int(off.max()) if off.size else 0
            if off.size and last + 4 <= a.size:
                block = int.from_bytes(a[last:last + 4].tobytes(), "little", signed=True)
                if 0 <= block <= a.size - last - 4:
                    b1 = last + 4 + block
            b1 = max(b0, b1)
            part = a[b0:b1] if b1 > b0 else np.zeros(1, np.uint8)
            d_bytes = torch.from_numpy(part if part.flags.writeable else part.copy()).to(dev)   # no host copy if it can be avoided
            d_off = torch.from_numpy((off - np.uint64(b0)).astype(np.int64)).to(dev)
            d_from = torch.from_numpy(np.ascontiguousarray(frm, np.int32).copy()).to(dev)
            smp.append((d_bytes, b1 - b0, d_off, d_from, int(off.size)))
        r = None if ref is None else _u8(ref)
        d_ref = None if r is None or r.size == 0 else torch.from_numpy(r.copy()).to(dev)
        torch.cuda.synchronize(dev)
        ns, nt, nn = self.count(smp[0], smp[1], d_ref, 0 if r is None else r.size, lo, hi, stream=stream)
        i32 = dict(dtype=torch.int32, device=dev)
        out = {"pos": torch.empty(max(1, ns), **i32), "ref": torch.empty(max(1, ns), dtype=torch.uint8, device=dev),
               "raw_t": torch.empty(max(1, ns), **i32), "raw_n": torch.empty(max(1, ns), **i32),
               "off_tumor": torch.empty(ns + 1, **i32), "off_normal": torch.empty(ns + 1, **i32),
               "reads_tumor": torch.empty(max(1, nt), **i32), "reads_normal": torch.empty(max(1, nn), **i32)}
        torch.cuda.synchronize(dev)
        self.fill(out["pos"], out["ref"], out["raw_t"], out["raw_n"], out["off_tumor"], out["off_normal"],
                  out["reads_tumor"], out["reads_normal"], ns, nt, nn, stream=stream)
        out["n_sites"] = ns
        out["n_reads"] = (nt, nn)
        out["_inputs"] = (smp, d_ref)          # the fill reads them: kept until the caller drops the dict
        return out

    def plan_device(self, data, n_bytes: int, n_ref: int, mask: int = -1, thresh: int = 0,
                    state: PileupState | None = None, cap: int | None = None, stream=None, cap_runs: int | None = None,
                    invalid_ok: bool = False):
        """ss_pileup_plan_device: pileup_plan over record bytes in device memory (a torch
        CUDA u8 tensor or a raw address, positioned after the header).  Returns
        (rec_off i64, from_ i32, tid i32 torch tensors trimmed to n, consumed, runs
        (SS_RUN_DTYPE), n_repaired); `state` is updated in place.  invalid_ok: after
        SS_E_INVAL return the records before the failing one (the code is then in
        self.last_plan_rc) instead of raising."""
        import torch
        dev = torch.device("cuda", self.device)
        if state is None:
            state = PileupState()
        if cap is None:
            cap = n_bytes // 36 + 1                # no record is shorter than 36 bytes
        if cap_runs is None:
            cap_runs = max(1, n_ref) + 16
        off = torch.empty(max(1, cap), dtype=torch.int64, device=dev)
        frm = torch.empty(max(1, cap), dtype=torch.int32, device=dev)
        tid = torch.empty(max(1, cap), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        sh = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
        n, used, n_runs, rep = C.c_uint32(), C.c_uint64(), C.c_uint32(), C.c_uint32()
        for attempt in range(2):
            runs = np.zeros(cap_runs, SS_RUN_DTYPE)
            st = PileupState.from_buffer_copy(state)
            rc = self.lib.ss_pileup_plan_device(self.h, self._p(data), n_bytes, n_ref, mask, thresh, C.byref(st),
                                                off.data_ptr(), frm.data_ptr(), tid.data_ptr(), cap, C.byref(n),
                                                C.byref(used), runs.ctypes.data, cap_runs, C.byref(n_runs),
                                                C.byref(rep), sh)
            if rc != SS_E_CAPACITY or attempt:
                break
            cap_runs = int(n_runs.value)           # the count needed
        self.last_plan_rc = rc
        if rc != SS_OK and not (rc == SS_E_INVAL and invalid_ok):
            raise SniperError(rc, "ss_pileup_plan_device")
        C.memmove(C.byref(state), C.byref(st), C.sizeof(st))
        k = int(n.value)
        return off[:k], frm[:k], tid[:k], int(used.value), runs[: n_runs.value].copy(), int(rep.value)

    def check(self):
        """Wait for the handle's work; SS_E_INVAL if a record of a device call failed
        validation; debug build: SS_E_CORRUPT if a guard band was overwritten."""
        _check(self.lib.ss_pileup_check(self.h), "ss_pileup_check")
