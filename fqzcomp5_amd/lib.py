"""ctypes binding of libfqz5_mi355x.so (include/fqz5_mi355x.h).

This is the only way the Python side reaches the codec: every call goes to
the HIP library.  There is no fallback — if the library or a GPU is missing
the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libfqz5_mi355x.so")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")

# helper contexts' streams need queues of their own (bench.py); effective
# only when nothing in the process has initialised HIP yet
# (the rule of capi.cpp's hw_queues_default: FQZ5_HW_QUEUES as given, else
# an unset value or HIP's default of 4 raised to 20, any other value kept)
if os.environ.get("FQZ5_HW_QUEUES"):
    os.environ["GPU_MAX_HW_QUEUES"] = os.environ["FQZ5_HW_QUEUES"]
elif os.environ.get("GPU_MAX_HW_QUEUES", "") in ("", "4"):
    os.environ["GPU_MAX_HW_QUEUES"] = "20"

_libc = C.CDLL(None)
_libc.free.argtypes = [C.c_void_p]


class RansJob(C.Structure):
    _fields_ = [("in_", C.c_void_p), ("out", C.c_void_p),
                ("in_size", C.c_uint32), ("out_cap", C.c_uint32),
                ("order", C.c_int32), ("out_size", C.c_uint32),
                ("status", C.c_int32), ("pad", C.c_int32)]


class FqzSlice(C.Structure):
    """fqz_slice (include/fqz5_mi355x.h; htscodecs fqzcomp_qual.h:59-64)."""
    _fields_ = [("num_records", C.c_int),
                ("len", C.POINTER(C.c_uint32)),
                ("flags", C.POINTER(C.c_uint32)),
                ("seq", C.POINTER(C.c_void_p))]


class FqzParam(C.Structure):
    """fqz_param (include/fqz5_mi355x.h; htscodecs fqzcomp_qual.h:92-125)."""
    _fields_ = [("context", C.c_uint16), ("pflags", C.c_uint),
                ("do_sel", C.c_uint), ("do_dedup", C.c_uint),
                ("store_qmap", C.c_uint), ("fixed_len", C.c_uint),
                ("use_qtab", C.c_ubyte), ("use_dtab", C.c_ubyte), ("use_ptab", C.c_ubyte),
                ("qbits", C.c_uint), ("qloc", C.c_uint),
                ("pbits", C.c_uint), ("ploc", C.c_uint),
                ("dbits", C.c_uint), ("dloc", C.c_uint),
                ("sbits", C.c_uint), ("sloc", C.c_uint),
                ("bbits", C.c_uint), ("bloc", C.c_uint), ("boff", C.c_uint),
                ("max_sym", C.c_int), ("nsym", C.c_int), ("max_sel", C.c_int),
                ("qmap", C.c_uint * 256), ("qtab", C.c_uint * 256),
                ("ptab", C.c_uint * 1024), ("dtab", C.c_uint * 256),
                ("qshift", C.c_int), ("pshift", C.c_int), ("dshift", C.c_int),
                ("sshift", C.c_int), ("qmask", C.c_uint),
                ("do_r2", C.c_int), ("do_qa", C.c_int)]


class FqzGParams(C.Structure):
    """fqz_gparams (include/fqz5_mi355x.h; fqzcomp_qual.h:129-139)."""
    _fields_ = [("vers", C.c_int), ("gflags", C.c_uint), ("nparam", C.c_int),
                ("max_sel", C.c_int), ("stab", C.c_uint * 256), ("max_sym", C.c_int),
                ("p", C.POINTER(FqzParam))]


def fqz_gparams(gflags: int, params: list[dict], max_sel: int = 0, stab=None,
                max_sym: int | None = None, vers: int = 5) -> FqzGParams:
    """A caller's fqz_gparams from plain values: one dict per parameter block,
    keyed by the fqz_param field names (tables as sequences, missing fields
    zero).  The blocks stay alive with the returned structure."""
    blocks = (FqzParam * len(params))()
    for b, d in zip(blocks, params):
        for k, v in d.items():
            if k in ("qmap", "qtab", "ptab", "dtab"):
                arr = getattr(b, k)
                for i, x in enumerate(v):
                    arr[i] = int(x)
            else:
                setattr(b, k, int(v))
    gp = FqzGParams(vers, gflags, len(params), max_sel)
    for i, x in enumerate(stab if stab is not None else []):
        gp.stab[i] = int(x)
    gp.max_sym = max(b.max_sym for b in blocks) if max_sym is None else max_sym
    gp.p = C.cast(blocks, C.POINTER(FqzParam))
    gp._blocks = blocks
    return gp


def fqz_gparams_state(gp: FqzGParams) -> dict:
    """What fqz_compress leaves in a caller's block: gflags, and per parameter
    block the sequence-context bits and the (shifted) position / delta tables."""
    return {"gflags": int(gp.gflags),
            "blocks": [{"bbits": int(gp.p[k].bbits), "bloc": int(gp.p[k].bloc),
                        "ptab": list(gp.p[k].ptab), "dtab": list(gp.p[k].dtab)}
                       for k in range(gp.nparam)]}


class NativeError(RuntimeError):
    pass


_lib = None


def load() -> C.CDLL:
    """Load the native library (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("FQZ5_LIB_VARIANT") or LIB_PATH   # tools/build_variant.sh
    # torch bundles its own HIP runtime, and the package's device buffers
    # (sections.py, fqz5file.py) are torch tensors: its runtime must own the
    # device before this library's runtime starts (started the other way
    # round, torch later finds no GPU)
    try:
        import torch
    except ImportError:
        torch = None
    if torch is not None and torch.cuda.is_available():
        torch.cuda.init()
    if not os.path.exists(path):
        raise NativeError(f"{path} missing: run __graft_entry__.build()")
    lib = C.CDLL(path)
    lib.fqz5_set_hedge.restype = C.c_int
    lib.fqz5_set_hedge.argtypes = [C.c_int]
    lib.fqz5_set_dec_small.restype = C.c_int
    lib.fqz5_set_dec_small.argtypes = [C.c_int]
    lib.fqz5_set_host_decode.restype = C.c_int
    lib.fqz5_set_host_decode.argtypes = [C.c_int]
    lib.fqz5_host_threads.restype = C.c_int
    lib.fqz5_host_threads.argtypes = []
    lib.fqz5_set_hot_min.restype = C.c_uint
    lib.fqz5_set_hot_min.argtypes = [C.c_uint]
    lib.rans_compress_bound_4x16.restype = C.c_uint
    lib.rans_compress_bound_4x16.argtypes = [C.c_uint, C.c_int]
    lib.rans_compress_to_4x16.restype = C.c_void_p
    lib.rans_compress_to_4x16.argtypes = [C.c_char_p, C.c_uint, C.c_void_p,
                                          C.POINTER(C.c_uint), C.c_int]
    lib.rans_compress_4x16.restype = C.c_void_p
    lib.rans_compress_4x16.argtypes = [C.c_char_p, C.c_uint,
                                       C.POINTER(C.c_uint), C.c_int]
    lib.rans_uncompress_to_4x16.restype = C.c_void_p
    lib.rans_uncompress_to_4x16.argtypes = [C.c_char_p, C.c_uint, C.c_void_p,
                                            C.POINTER(C.c_uint)]
    lib.rans_uncompress_4x16.restype = C.c_void_p
    lib.rans_uncompress_4x16.argtypes = [C.c_char_p, C.c_uint,
                                         C.POINTER(C.c_uint)]
    lib.fqz5_rans_compress_batch.restype = C.c_int
    lib.fqz5_rans_compress_batch.argtypes = [C.POINTER(RansJob), C.c_int]
    lib.fqz5_rans_uncompress_batch.restype = C.c_int
    lib.fqz5_rans_uncompress_batch.argtypes = [C.POINTER(RansJob), C.c_int]
    lib.fqz5_stream.restype = C.c_void_p
    lib.fqz5_stream_wait.restype = C.c_int
    lib.fqz5_stream_wait.argtypes = [C.c_void_p]
    lib.fqz5_device_ok.restype = C.c_int
    lib.fqz5_last_error.restype = C.c_char_p
    lib.fqz_compress.restype = C.c_void_p
    lib.fqz_compress.argtypes = [C.c_int, C.POINTER(FqzSlice), C.c_char_p, C.c_size_t,
                                 C.POINTER(C.c_size_t), C.c_int, C.c_void_p]
    lib.fqz_decompress.restype = C.c_void_p
    lib.fqz_decompress.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t),
                                   C.POINTER(C.c_int), C.c_int, C.POINTER(FqzSlice)]
    lib.arith_compress_bound.restype = C.c_uint
    lib.arith_compress_bound.argtypes = [C.c_uint, C.c_int]
    lib.arith_compress_to.restype = C.c_void_p
    lib.arith_compress_to.argtypes = [C.c_char_p, C.c_uint, C.c_void_p,
                                      C.POINTER(C.c_uint), C.c_int]
    lib.arith_compress.restype = C.c_void_p
    lib.arith_compress.argtypes = [C.c_char_p, C.c_uint, C.POINTER(C.c_uint), C.c_int]
    lib.arith_uncompress_to.restype = C.c_void_p
    lib.arith_uncompress_to.argtypes = [C.c_char_p, C.c_uint, C.c_void_p,
                                        C.POINTER(C.c_uint)]
    lib.arith_uncompress.restype = C.c_void_p
    lib.arith_uncompress.argtypes = [C.c_char_p, C.c_uint, C.POINTER(C.c_uint)]
    lib.fqz5_crc32.restype = C.c_ulong
    lib.fqz5_crc32.argtypes = [C.c_ulong, C.c_char_p, C.c_uint]
    lib.fqz5_crc32_dev.restype = C.c_int
    lib.fqz5_crc32_dev.argtypes = [C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32)]
    lib.fqz5_seq_encode.restype = C.c_void_p
    lib.fqz5_seq_encode.argtypes = [C.c_char_p, C.c_uint, C.POINTER(C.c_uint32), C.c_int,
                                    C.c_int, C.c_int, C.POINTER(C.c_uint)]
    lib.fqz5_seq_decode.restype = C.c_void_p
    lib.fqz5_seq_decode.argtypes = [C.c_char_p, C.c_uint, C.POINTER(C.c_uint32), C.c_int,
                                    C.c_int, C.c_int, C.c_uint]
    lib.fqz5_seq_decode_host.restype = C.c_void_p
    lib.fqz5_seq_decode_host.argtypes = [C.c_char_p, C.c_uint, C.POINTER(C.c_uint32), C.c_int,
                                    C.c_int, C.c_int, C.c_uint]
    lib.fqz5_fqz_decompress_host.restype = C.c_void_p
    lib.fqz5_fqz_decompress_host.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t),
                                   C.POINTER(C.c_int), C.c_int, C.POINTER(FqzSlice)]
    _lib = lib
    return lib


def last_error() -> str:
    return load().fqz5_last_error().decode()


def fqz_div_selftest() -> int:
    """Mismatches of the fqz decoder's division on the device (0 expected)."""
    so = load()
    so.fqz5_fqz_div_selftest.restype = C.c_long
    return int(so.fqz5_fqz_div_selftest())


def unrle_selftest(runs: bytes, nlit: int, nout: int, o: int = 0):
    """The RLE expansion's run arithmetic on the host (fqz5_unrle_selftest):
    (end offset saturated at nout + 1, write-loop trips, longest fill)."""
    so = load()
    so.fqz5_unrle_selftest.restype = C.c_int
    so.fqz5_unrle_selftest.argtypes = [C.c_char_p, C.c_uint, C.c_uint, C.c_uint, C.c_uint,
                                       C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 3)()
    if so.fqz5_unrle_selftest(bytes(runs), len(runs), nlit, nout, o, out):
        raise NativeError("fqz5_unrle_selftest: a fill passes nout")
    return int(out[0]), int(out[1]), int(out[2])


def device_ok() -> bool:
    return bool(load().fqz5_device_ok())


def arena_bytes() -> int:
    """Device bytes the arenas hold, process-wide (fqz5_arena_bytes)."""
    so = load()
    so.fqz5_arena_bytes.restype = C.c_uint64
    return int(so.fqz5_arena_bytes())


def arena_peak(reset: bool = False) -> int:
    """The most device bytes the arenas held since the last reset
    (fqz5_arena_peak)."""
    so = load()
    so.fqz5_arena_peak.restype = C.c_uint64
    so.fqz5_arena_peak.argtypes = [C.c_int]
    return int(so.fqz5_arena_peak(1 if reset else 0))


def arena_use_peak(reset: bool = False) -> int:
    """The most device bytes in use at once (held minus the pool's idle
    chunks) since the last reset (fqz5_arena_use_peak)."""
    so = load()
    so.fqz5_arena_use_peak.restype = C.c_uint64
    so.fqz5_arena_use_peak.argtypes = [C.c_int]
    return int(so.fqz5_arena_use_peak(1 if reset else 0))


def header_symbols() -> list[str]:
    """Function names declared in include/*.h."""
    import glob
    import re
    txt = "".join(open(f).read() for f in sorted(glob.glob(os.path.join(INCLUDE, "*.h"))))
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b([a-z_0-9]+)\s*\(", txt))
                  - {"if", "sizeof", "return"})


def compress_bound(n: int, order: int) -> int:
    return load().rans_compress_bound_4x16(n, order)


def rans_compress(data: bytes, order: int) -> bytes:
    """rans_compress_4x16 on the GPU (host buffers)."""
    lib = load()
    n = C.c_uint(0)
    p = lib.rans_compress_4x16(bytes(data), len(data), C.byref(n), order)
    if not p:
        raise NativeError("rans_compress_4x16 failed: " + last_error())
    out = C.string_at(p, n.value)
    _libc.free(p)
    return out


def rans_compress_to(data: bytes, order: int, cap: int) -> bytes | None:
    """rans_compress_to_4x16 with a caller buffer of `cap` bytes."""
    lib = load()
    buf = C.create_string_buffer(max(cap, 1))
    n = C.c_uint(cap)
    p = lib.rans_compress_to_4x16(bytes(data), len(data), buf, C.byref(n),
                                  order)
    if not p:
        return None
    return buf.raw[:n.value]


def rans_uncompress(comp: bytes) -> bytes:
    lib = load()
    n = C.c_uint(0)
    p = lib.rans_uncompress_4x16(bytes(comp), len(comp), C.byref(n))
    if not p:
        raise NativeError("rans_uncompress_4x16 failed: " + last_error())
    out = C.string_at(p, n.value)
    _libc.free(p)
    return out


def rans_chain_counts() -> tuple[int, int]:
    """Plain rANS chains placed so far: (on host cores, on the GPU)."""
    c = (C.c_uint64 * 2)()
    so = load()
    so.fqz5_rans_chain_counts.restype = None
    so.fqz5_rans_chain_counts.argtypes = [C.POINTER(C.c_uint64)]
    so.fqz5_rans_chain_counts(c)
    return int(c[0]), int(c[1])


def set_host_encode(mode: int) -> int:
    """fqz5_set_host_encode: where the compressor runs its bare NX = 4 chains
    (0 GPU, 1 host, 2 by cost, 3 every other one); the previous mode."""
    so = load()
    so.fqz5_set_host_encode.restype = C.c_int
    so.fqz5_set_host_encode.argtypes = [C.c_int]
    return int(so.fqz5_set_host_encode(mode))


def set_x32_group_min(n: int) -> int:
    """fqz5_set_x32_group_min: 32-state encoder chains of n symbols and more
    run as lane groups (k_enc_chain_x32g); the previous threshold."""
    so = load()
    so.fqz5_set_x32_group_min.restype = C.c_uint64
    so.fqz5_set_x32_group_min.argtypes = [C.c_uint64]
    return int(so.fqz5_set_x32_group_min(n))


def rans_enc_chain_counts() -> tuple[int, int]:
    """Encoder chains placed so far: (on host cores, on the GPU)."""
    c = (C.c_uint64 * 2)()
    so = load()
    so.fqz5_rans_enc_chain_counts.restype = None
    so.fqz5_rans_enc_chain_counts.argtypes = [C.POINTER(C.c_uint64)]
    so.fqz5_rans_enc_chain_counts(c)
    return int(c[0]), int(c[1])


def rans_variant_counts() -> tuple[dict[str, int], dict[str, int], dict[str, int]]:
    """fqz5_rans_variant_counts: GPU-launched rANS chain jobs so far by the
    kernel body that ran them, as (decoder, decoder jobs launched in several
    hedged copies, encoder), each keyed by fqz5_rans_variant_name."""
    so = load()
    so.fqz5_rans_variant_counts.restype = None
    so.fqz5_rans_variant_counts.argtypes = [C.POINTER(C.c_uint64)] * 3 + [C.POINTER(C.c_int)] * 2
    so.fqz5_rans_variant_name.restype = C.c_char_p
    so.fqz5_rans_variant_name.argtypes = [C.c_int, C.c_int]
    nd, ne = C.c_int(0), C.c_int(0)
    so.fqz5_rans_variant_counts(None, None, None, C.byref(nd), C.byref(ne))
    dec, hed, enc = (C.c_uint64 * nd.value)(), (C.c_uint64 * nd.value)(), (C.c_uint64 * ne.value)()
    so.fqz5_rans_variant_counts(dec, hed, enc, None, None)
    dn = [so.fqz5_rans_variant_name(0, i).decode() for i in range(nd.value)]
    en = [so.fqz5_rans_variant_name(1, i).decode() for i in range(ne.value)]
    return ({k: int(v) for k, v in zip(dn, dec)}, {k: int(v) for k, v in zip(dn, hed)},
            {k: int(v) for k, v in zip(en, enc)})


FQZ_PATH_NAMES = (["dec_ne%d_%s_%s" % (1 + (v >> 2), "seq" if v & 2 else "noseq",
                                       "qid" if v & 1 else "qtab") for v in range(8)] +
                  ["dec_small", "dec_small_dt", "map_all", "map_recs", "dups", "revs",
                   "relaunched", "enc_serial"])


def fqz_path_counts() -> dict[str, int]:
    """fqz5_fqz_path_counts: fqz blocks so far per decoder variant (the general
    decoder by model registers, sequence context and shared qtab; the small
    one without and with delta terms), per fix-up kernel, relaunched with
    longer record lists, and encoded by the serial kernel; "enc_parallel" the
    blocks the parallel encoder took."""
    so = load()
    so.fqz5_fqz_path_counts.restype = C.c_int
    so.fqz5_fqz_path_counts.argtypes = [C.POINTER(C.c_uint64), C.c_int]
    names = FQZ_PATH_NAMES + ["enc_parallel"]
    out = (C.c_uint64 * len(names))()
    if so.fqz5_fqz_path_counts(out, len(names)) != len(names):
        raise NativeError("fqz5_fqz_path_counts: the library counts other paths")
    return {k: int(v) for k, v in zip(names, out)}


def rans_enc_chain_host(data: bytes, order: int, bits: int, freq) -> list[int] | None:
    """fqz5_rans_enc_chain_host: the bare encoder chain's checkpoints (u32
    words) on a host core (no GPU).  freq: 256 frequencies (order 0) or
    256 x 256, row = context byte (order 1), flat; None where it refuses."""
    want = 256 if order == 0 else 65536
    fa = (C.c_uint32 * want)(*[int(x) for x in freq])
    n = C.c_size_t(0)
    so = load()
    so.fqz5_rans_enc_chain_host.restype = C.c_void_p
    so.fqz5_rans_enc_chain_host.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int,
                                            C.POINTER(C.c_uint32), C.POINTER(C.c_size_t)]
    p = so.fqz5_rans_enc_chain_host(bytes(data), len(data), order, bits, fa, C.byref(n))
    if not p:
        return None
    out = list((C.c_uint32 * n.value).from_address(p))
    _libc.free(p)
    return out


def rans_dec_host(comp: bytes, cap: int) -> bytes | None:
    """fqz5_rans_dec_host: a plain order-0 / order-1 4x16 stream on a host
    core (no GPU); None where it fails or refuses the order byte."""
    buf = C.create_string_buffer(max(cap, 1))
    n = C.c_size_t(0)
    so = load()
    so.fqz5_rans_dec_host.restype = C.c_int
    so.fqz5_rans_dec_host.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                      C.POINTER(C.c_size_t)]
    if so.fqz5_rans_dec_host(bytes(comp), len(comp), buf, cap, C.byref(n)):
        return None
    return buf.raw[:n.value]


def host_plan(n, kind, threads: int, core_ns=None) -> list[int]:
    """host::plan: 1 per chain placed on a host core, 0 for the GPU."""
    cnt = len(n)
    na = (C.c_uint64 * max(cnt, 1))(*[int(x) for x in n])
    ka = (C.c_int * max(cnt, 1))(*[int(x) for x in kind])
    ca = None if core_ns is None else (C.c_double * threads)(*[float(x) for x in core_ns])
    out = C.create_string_buffer(max(cnt, 1))
    so = load()
    so.fqz5_host_plan.restype = None
    so.fqz5_host_plan.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.c_int, C.c_int,
                                  C.POINTER(C.c_double), C.c_char_p]
    so.fqz5_host_plan(na, ka, cnt, threads, ca, out)
    return [out.raw[i] for i in range(cnt)]


def rans_uncompress_to(comp: bytes, size: int) -> bytes | None:
    lib = load()
    buf = C.create_string_buffer(max(size, 1))
    n = C.c_uint(size)
    p = lib.rans_uncompress_to_4x16(bytes(comp), len(comp), buf, C.byref(n))
    if not p:
        return None
    return buf.raw[:n.value]


def arith_compress(data: bytes, order: int, cap: int | None = None) -> bytes | None:
    """arith_compress (cap None) or arith_compress_to with a caller buffer
    of `cap` bytes, on the GPU; None where the reference returns NULL."""
    lib = load()
    if cap is None:
        n = C.c_uint(0)
        p = lib.arith_compress(bytes(data), len(data), C.byref(n), order)
        if not p:
            return None
        out = C.string_at(p, n.value)
        _libc.free(p)
        return out
    buf = C.create_string_buffer(max(cap, 1))
    n = C.c_uint(cap)
    p = lib.arith_compress_to(bytes(data), len(data), buf, C.byref(n), order)
    return None if not p else buf.raw[:n.value]


def arith_uncompress(comp: bytes, out_size: int | None = None) -> bytes | None:
    """arith_uncompress (out_size None) or arith_uncompress_to into a
    buffer of out_size bytes, on the GPU; None on failure."""
    lib = load()
    if out_size is None:
        n = C.c_uint(0)
        p = lib.arith_uncompress(bytes(comp), len(comp), C.byref(n))
        if not p:
            return None
        out = C.string_at(p, n.value)
        _libc.free(p)
        return out
    buf = C.create_string_buffer(max(out_size, 1))
    n = C.c_uint(out_size)
    p = lib.arith_uncompress_to(bytes(comp), len(comp), buf, C.byref(n))
    return None if not p else buf.raw[:n.value]


def compress_batch_dev(jobs: list[RansJob]) -> None:
    arr = (RansJob * len(jobs))(*jobs)
    if load().fqz5_rans_compress_batch(arr, len(jobs)) != 0:
        raise NativeError("fqz5_rans_compress_batch: " + last_error())
    for i, j in enumerate(jobs):
        j.out_size, j.status = arr[i].out_size, arr[i].status


def uncompress_batch_dev(jobs: list[RansJob]) -> None:
    arr = (RansJob * len(jobs))(*jobs)
    if load().fqz5_rans_uncompress_batch(arr, len(jobs)) != 0:
        raise NativeError("fqz5_rans_uncompress_batch: " + last_error())
    for i, j in enumerate(jobs):
        j.out_size, j.status = arr[i].out_size, arr[i].status


def _fqz_slice(lens, flags, seq: bytes | None):
    """Build an fqz_slice over numpy-like lens/flags (uint32, modified in
    place by fqz_compress as the reference does) and optional sequences."""
    import numpy as np
    lens = np.ascontiguousarray(lens, np.uint32)
    flags = np.ascontiguousarray(flags, np.uint32)
    nr = len(lens)
    keep = [lens, flags]
    S = None
    if seq is not None:
        sb = C.create_string_buffer(bytes(seq), len(seq) + 1)
        keep.append(sb)
        base = C.addressof(sb)
        offs = np.concatenate([[0], np.cumsum(lens.astype(np.int64))])
        S = (C.c_void_p * max(nr, 1))(*[base + int(o) for o in offs[:-1]])
        keep.append(S)
    s = FqzSlice(nr, lens.ctypes.data_as(C.POINTER(C.c_uint32)),
                 flags.ctypes.data_as(C.POINTER(C.c_uint32)), S)
    return s, keep, lens, flags


def fqz_compress(qual: bytes, lens, flags, strat: int, seq: bytes | None = None,
                 vers: int = 4, gp: FqzGParams | None = None) -> bytes:
    """fqz_compress on the GPU (host buffers; values are q-33).  gp: the
    caller's parameters (fqz_gparams()), edited in place as the reference does."""
    s, keep, _, _ = _fqz_slice(lens, flags, seq)
    n = C.c_size_t(0)
    p = load().fqz_compress(vers, C.byref(s), bytes(qual), len(qual), C.byref(n), strat,
                            C.byref(gp) if gp is not None else None)
    if not p:
        raise NativeError("fqz_compress failed: " + last_error())
    out = C.string_at(p, n.value)
    _libc.free(p)
    return out


def fqz_decompress(comp: bytes, lens=None, flags=None, seq: bytes | None = None,
                   host: bool = False):
    """fqz_decompress on the GPU (host=True: fqz5_fqz_decompress_host, the
    same decoder on a host core); returns (bytes, record lengths)."""
    import numpy as np
    lens = np.zeros(0, np.uint32) if lens is None else lens
    flags = np.zeros(len(lens), np.uint32) if flags is None else flags
    s, keep, lens_a, _ = _fqz_slice(lens, flags, seq)
    n = C.c_size_t(0)
    nl = len(lens_a)
    L = (C.c_int * max(nl, 1))()
    so = load()
    fn = so.fqz5_fqz_decompress_host if host else so.fqz_decompress
    p = fn(bytes(comp), len(comp), C.byref(n), L, nl, C.byref(s))
    if not p:
        raise NativeError("fqz_decompress failed: " + last_error())
    out = C.string_at(p, n.value)
    _libc.free(p)
    return out, [L[i] for i in range(nl)]


def _seq_lens(lens):
    lens = [int(x) for x in lens] or [0]
    return (C.c_uint32 * len(lens))(*lens), len(lens)


def seq_encode(seq: bytes, lens, both: int, k: int) -> bytes:
    """fqz5_seq_encode (encode_seq, fqzcomp5.c:1073) on the GPU."""
    la, nr = _seq_lens(lens)
    n = C.c_uint(0)
    p = load().fqz5_seq_encode(bytes(seq), len(seq), la, nr, both, k, C.byref(n))
    if not p:
        raise NativeError("fqz5_seq_encode failed: " + last_error())
    out = C.string_at(p, n.value)
    _libc.free(p)
    return out


def seq_decode(comp: bytes, lens, both: int, k: int, out_size: int, host: bool = False) -> bytes:
    """fqz5_seq_decode (decode_seq, fqzcomp5.c:1272) on the GPU (host=True:
    fqz5_seq_decode_host on a host core)."""
    la, nr = _seq_lens(lens)
    so = load()
    fn = so.fqz5_seq_decode_host if host else so.fqz5_seq_decode
    p = fn(bytes(comp), len(comp), la, nr, both, k, out_size)
    if not p:
        raise NativeError("fqz5_seq_decode failed: " + last_error())
    out = C.string_at(p, out_size)
    _libc.free(p)
    return out


SEQ_PATH_NAMES = (["dec_lookahead", "dec_one_step", "model_events"] +
                  ["model_span_%d" % (256 * (i + 1)) for i in range(16)])


def seq_path_counts() -> dict[str, int]:
    """fqz5_seq_path_counts: sequence-model decoder jobs per kernel and
    model-pass launches per tile width (or in the per-event form)."""
    so = load()
    so.fqz5_seq_path_counts.restype = C.c_int
    so.fqz5_seq_path_counts.argtypes = [C.POINTER(C.c_uint64), C.c_int]
    out = (C.c_uint64 * len(SEQ_PATH_NAMES))()
    if so.fqz5_seq_path_counts(out, len(SEQ_PATH_NAMES)) != len(SEQ_PATH_NAMES):
        raise NativeError("fqz5_seq_path_counts: the library counts other paths")
    return {k: int(v) for k, v in zip(SEQ_PATH_NAMES, out)}


def seq_decode_many(streams, in_offset: int = 0) -> list[tuple[int, bytes]]:
    """fqz5_seq_decode_many: streams of (comp, lens, both, k, out_size), packed
    back to back on the device from in_offset (0..15) past a 16-byte boundary
    and decoded in one batch; (status, bytes) per stream."""
    so = load()
    n = len(streams)
    PU, PB = C.POINTER(C.c_uint32), C.POINTER(C.c_ubyte)
    so.fqz5_seq_decode_many.restype = C.c_int
    so.fqz5_seq_decode_many.argtypes = [C.c_int, C.POINTER(C.c_char_p), PU, C.POINTER(PU),
                                        C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                        PU, C.c_int, C.POINTER(PB), C.POINTER(C.c_int)]
    comps = [bytes(s[0]) for s in streams]
    lens = [_seq_lens(s[1]) for s in streams]
    outs = [(C.c_ubyte * max(int(s[4]), 1))() for s in streams]
    ints = lambda v: (C.c_int * n)(*v)
    status = ints([1] * n)
    rc = so.fqz5_seq_decode_many(
        n, (C.c_char_p * n)(*comps), (C.c_uint32 * n)(*[len(c) for c in comps]),
        (PU * n)(*[C.cast(la, PU) for la, _ in lens]), ints([nr for _, nr in lens]),
        ints([int(s[2]) for s in streams]), ints([int(s[3]) for s in streams]),
        (C.c_uint32 * n)(*[int(s[4]) for s in streams]), in_offset,
        (PB * n)(*[C.cast(o, PB) for o in outs]), status)
    if rc != 0:
        raise NativeError("fqz5_seq_decode_many failed: " + last_error())
    return [(int(status[i]), bytes(outs[i])[:int(streams[i][4])]) for i in range(n)]


def lzp(data: bytes) -> bytes:
    """fqz5_lzp (lzp16e.c:113 lzp) on the GPU."""
    so = load()
    so.fqz5_lzp.restype = C.c_int
    so.fqz5_lzp.argtypes = [C.c_char_p, C.c_int, C.c_void_p]
    buf = C.create_string_buffer(3 * len(data) + 16)
    n = so.fqz5_lzp(bytes(data), len(data), buf)
    if n < 0:
        raise NativeError("fqz5_lzp failed: " + last_error())
    return buf.raw[:n]


def unlzp(data: bytes, out_cap: int) -> bytes | None:
    """fqz5_unlzp (lzp16e.c:166 unlzp) on the GPU; None if the stream is
    damaged or decodes to more than out_cap bytes."""
    so = load()
    so.fqz5_unlzp.restype = C.c_int
    so.fqz5_unlzp.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_int]
    buf = C.create_string_buffer(max(out_cap, 1))
    n = so.fqz5_unlzp(bytes(data), len(data), buf, out_cap)
    return None if n < 0 else buf.raw[:n]


def unlzp_host(data: bytes, out_cap: int) -> bytes | None:
    """fqz5_unlzp_host: unlzp on a host core (no GPU); None where fqz5_unlzp
    fails.  The buffer has out_cap bytes and a guard after them, which must
    come back untouched."""
    so = load()
    so.fqz5_unlzp_host.restype = C.c_int
    so.fqz5_unlzp_host.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                   C.POINTER(C.c_size_t)]
    guard = b"\xa5" * 64
    buf = C.create_string_buffer(out_cap + len(guard))
    buf[out_cap:out_cap + len(guard)] = guard
    n = C.c_size_t(0)
    rc = so.fqz5_unlzp_host(bytes(data), len(data), buf, out_cap, C.byref(n))
    if buf.raw[out_cap:out_cap + len(guard)] != guard or n.value > out_cap:
        raise NativeError("fqz5_unlzp_host wrote past out_cap")
    return None if rc else buf.raw[:n.value]


def crc32(data: bytes, crc: int = 0) -> int:
    """zlib.crc32 computed on the GPU (fqz5_crc32, host buffer)."""
    return int(load().fqz5_crc32(crc, bytes(data), len(data)))


def stream_wait(stream: int) -> None:
    """Order the library's stream after the work enqueued so far on
    `stream` (a hipStream_t as int, e.g. torch's Stream.cuda_stream):
    fqz5_stream_wait, the ordering contract of the device-pointer calls."""
    if load().fqz5_stream_wait(C.c_void_p(stream)):
        raise NativeError("fqz5_stream_wait failed: " + last_error())


def after_torch(dev=None) -> None:
    """The ordering contract of the device-pointer calls for buffers torch
    made: the calling thread's library streams (and its helper contexts')
    wait, device-side, for the work enqueued so far on torch's current
    stream of the current device and, when `dev` (the device of the buffers
    the call reads) is another one, on that device's current stream too (a
    torch.cat output, a buffer the caching allocator reused).  Called before
    every device-pointer entry point of sections / fqz5file; a no-op while
    torch has not initialised the GPU."""
    import sys
    torch = sys.modules.get("torch")
    if torch is None or not torch.cuda.is_initialized():
        return
    cur = torch.cuda.current_device()
    stream_wait(torch.cuda.current_stream(cur).cuda_stream)
    if dev is not None:
        d = torch.device(dev)
        if d.type == "cuda" and d.index is not None and d.index != cur:
            stream_wait(torch.cuda.current_stream(d).cuda_stream)


def crc32_dev(ptr: int, n: int, crc: int = 0) -> int:
    """crc32 of n device bytes at ptr (fqz5_crc32_dev)."""
    out = C.c_uint32(0)
    if load().fqz5_crc32_dev(crc, C.c_void_p(ptr), n, C.byref(out)):
        raise NativeError("fqz5_crc32_dev failed: " + last_error())
    return int(out.value)


def tok3_encode(names: bytes, level: int, use_arith: int = 0):
    """tok3_encode_names (tokenise_name3.c:1451): tokenised on the host, the
    token streams entropy coded as one GPU batch.  Works on a private copy
    of `names` (the codec rewrites terminators): (stream, last_start), or
    None where the reference returns NULL."""
    so = load()
    f = so.tok3_encode_names
    f.restype = C.c_void_p
    f.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int),
                  C.POINTER(C.c_int)]
    buf = C.create_string_buffer(bytes(names), max(len(names), 1))
    n, ls = C.c_int(0), C.c_int(-1)
    p = f(buf, len(names), level, use_arith, C.byref(n), C.byref(ls))
    if not p:
        return None
    out = C.string_at(p, n.value)
    _libc.free(p)
    return out, ls.value


def tok3_decode(comp: bytes) -> bytes | None:
    """tok3_decode_names (tokenise_name3.c:1679): the '\\0'-terminated
    names, or None on a malformed stream."""
    so = load()
    f = so.tok3_decode_names
    f.restype = C.c_void_p
    f.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32)]
    n = C.c_uint32(0)
    p = f(bytes(comp), len(comp), C.byref(n))
    if not p:
        return None
    out = C.string_at(p, n.value)
    _libc.free(p)
    return out
