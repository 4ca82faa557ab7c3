"""kzg-grandsums-study_amd — MI355X-native KZG grand-sum / grand-product prover (host mirror).

Python mirror of the reference's module API (xavi-pinsach/kzg-grandsums-study):

    prover(pTauFilename, evalsFs, evalsTs, evalsSelF=None, evalsSelT=None) -> proof
        src/grandsum/mset_eq_kzg_prover.js:12  -> grandsum_prover
        src/grandproduct/mset_eq_kzg_prover.js:12 -> grandproduct_prover
    lookup_prover(pTauFilename, evalsFs, evalsTs, evalsSelF, evalsMulT) -> proof
        test/lookup_kzg_grandsum.test.js:24-44 (commented out in the reference) -> KGS_LOOKUP

over the C-ABI library lib/libkgs.so (include/kgs.h; HIP kernels for gfx950). The JavaScript
drop-in modules (js/) bind the same library through an N-API addon. There is NO CPU fallback:
if the HIP library cannot be loaded the import raises.

Input/ownership conventions follow the reference exactly: F/T evaluations are
32 B LE standard-form buffers that are overwritten with their Montgomery form (prover.js:147-148);
selectors are Montgomery buffers; the proof is {"commitments": {name: 64 B LEM},
"evaluations": {name: 32 B LE Montgomery}}.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KGS_LIB") or os.path.join(_HERE, "lib", "libkgs.so")

GRANDSUM = 0
GRANDPRODUCT = 1
LOOKUP = 2
# kgs_ntt_ex flags (include/kgs.h KGS_NTT_*)
NTT_INVERSE, NTT_COSET, NTT_BITREV, NTT_NO_SCALE, NTT_INPLACE, NTT_INFLIGHT = 1, 2, 4, 8, 16, 32

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
FR_ONE_MONT = ((1 << 256) % R).to_bytes(32, "little")

_lib = None


class KgsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


KGS_E_RANGE = -9


class ProofRef(ctypes.Structure):
    """kgs_proof_ref_t (include/kgs.h)."""
    _fields_ = [("kind", ctypes.c_int), ("nbits", ctypes.c_int), ("npols", ctypes.c_int), ("selected", ctypes.c_int),
                ("commitments", ctypes.c_void_p), ("evaluations", ctypes.c_void_p)]


class BatchDiag(ctypes.Structure):
    """kgs_batch_diag_t (include/kgs.h)."""
    _fields_ = [("weights_out", ctypes.c_void_p), ("folded_out", ctypes.c_void_p), ("pairing_checks", ctypes.c_uint32),
                ("terms", ctypes.c_uint32), ("on_gpu", ctypes.c_int), ("fold_ms", ctypes.c_double),
                ("pairing_ms", ctypes.c_double)]


class CosetBatchDiag(ctypes.Structure):
    """kgs_coset_batch_diag_t (include/kgs.h)."""
    _fields_ = [("rho_out", ctypes.c_void_p), ("folded_out", ctypes.c_void_p), ("interp_out", ctypes.c_void_p),
                ("pairing_checks", ctypes.c_uint32), ("on_gpu", ctypes.c_int), ("hash_ms", ctypes.c_double),
                ("fold_ms", ctypes.c_double), ("pairing_ms", ctypes.c_double)]


MAX_ARGS = 16


class ArgShape(ctypes.Structure):
    """kgs_arg_shape_t (include/kgs.h)."""
    _fields_ = [("kind", ctypes.c_int), ("npols", ctypes.c_int), ("selected", ctypes.c_int)]


class Arg(ctypes.Structure):
    """kgs_arg_t (include/kgs.h)."""
    _fields_ = [("kind", ctypes.c_int), ("npols", ctypes.c_int), ("evals_f", ctypes.POINTER(ctypes.c_void_p)),
                ("evals_t", ctypes.POINTER(ctypes.c_void_p)), ("sel_f", ctypes.c_void_p), ("sel_t", ctypes.c_void_p)]


class QuotArg(ctypes.Structure):
    """kgs_quot_arg_t (include/kgs.h)."""
    _fields_ = [("kind", ctypes.c_int), ("S", ctypes.c_void_p), ("F", ctypes.c_void_p), ("T", ctypes.c_void_p),
                ("sel_f", ctypes.c_void_p), ("sel_t", ctypes.c_void_p)]


QUOT_FUSED = 1  # kgs_quotient_ex flag (include/kgs.h KGS_QUOT_FUSED)


class RangeError(ValueError):
    """What the reference's JavaScript throws as a RangeError ("offset is out of bounds": its divZh on a
    zero quotient, polynomial.js:857,884) — raised in reference-quirks mode only (include/kgs.h
    kgs_ctx_set_reference_quirks)."""


def _semantic(e):
    """KgsError from the library -> the exception the reference's prover would throw."""
    return RangeError(str(e)) if e.code == KGS_E_RANGE else ValueError(str(e))


def lib():
    """Load lib/libkgs.so (raises if it is missing: the HIP path is the only path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"HIP library not built: {LIB_PATH} (run __graft_entry__.build())")
        L = ctypes.CDLL(LIB_PATH)
        c_u8p = ctypes.c_void_p
        L.kgs_last_error.restype = ctypes.c_char_p
        L.kgs_version.restype = ctypes.c_char_p
        L.kgs_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        L.kgs_ctx_destroy.argtypes = [ctypes.c_void_p]
        L.kgs_ctx_destroy.restype = None
        L.kgs_srs_load_ptau.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
        L.kgs_srs_load_ptau_slice.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.kgs_srs_slice_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                         ctypes.POINTER(ctypes.c_uint64)]
        L.kgs_ptau_power.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
        L.kgs_device_count.argtypes = [ctypes.POINTER(ctypes.c_int)]
        L.kgs_srs_load_points.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int]
        L.kgs_srs_info.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64),
                                   ctypes.POINTER(ctypes.c_int)]
        L.kgs_ptau_read_tau_g2.argtypes = [ctypes.c_char_p, c_u8p]
        L.kgs_ptau_write_synthetic.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, c_u8p]
        PP = ctypes.POINTER(ctypes.c_void_p)
        L.kgs_prove.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, PP, PP, c_u8p, c_u8p,
                                PP, PP, c_u8p, c_u8p]
        L.kgs_prove_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, PP, PP,
                                       ctypes.c_void_p, ctypes.c_void_p, c_u8p, c_u8p]
        L.kgs_proof_shape.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                      ctypes.POINTER(ctypes.c_int)]
        L.kgs_host_register.argtypes = [c_u8p, ctypes.c_uint64]
        L.kgs_host_unregister.argtypes = [c_u8p]
        L.kgs_last_timing.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int]
        L.kgs_ctx_idle.argtypes = [ctypes.c_void_p]
        L.kgs_fr_to_mont.argtypes = [ctypes.c_void_p, c_u8p, c_u8p, ctypes.c_uint64]
        L.kgs_fr_from_mont.argtypes = [ctypes.c_void_p, c_u8p, c_u8p, ctypes.c_uint64]
        L.kgs_fr_batch_inverse.argtypes = [ctypes.c_void_p, c_u8p, c_u8p, ctypes.c_uint64]
        L.kgs_ntt.argtypes = [ctypes.c_void_p, c_u8p, c_u8p, ctypes.c_int, ctypes.c_int]
        L.kgs_ntt_ex.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, c_u8p, ctypes.c_int, ctypes.c_int]
        L.kgs_ntt_blocks.argtypes = [ctypes.c_void_p, c_u8p, c_u8p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.kgs_msm.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, c_u8p]
        L.kgs_grand_build.argtypes = [ctypes.c_void_p, ctypes.c_int, c_u8p, c_u8p, c_u8p, c_u8p, c_u8p,
                                      ctypes.c_uint64, c_u8p]
        L.kgs_quotient_ex.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(QuotArg), ctypes.c_int,
                                      c_u8p, c_u8p, c_u8p, ctypes.c_int, c_u8p]
        L.kgs_divcheck.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, c_u8p, c_u8p, c_u8p, c_u8p, c_u8p,
                                   c_u8p, c_u8p, c_u8p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_int)]
        L.kgs_lincomb.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64),
                                  c_u8p, ctypes.c_int, c_u8p, ctypes.c_uint64, c_u8p]
        L.kgs_poly_eval.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, c_u8p, c_u8p]
        L.kgs_poly_div_x_sub.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, c_u8p, c_u8p]
        L.kgs_lookup_multiplicities.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, PP, PP, c_u8p, c_u8p]
        L.kgs_lookup_multiplicities_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, PP, PP,
                                                       ctypes.c_void_p, ctypes.c_void_p]
        L.kgs_keccak256.argtypes = [c_u8p, ctypes.c_uint64, c_u8p]
        L.kgs_bench_msm.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                    ctypes.POINTER(ctypes.c_double)]
        L.kgs_bench_msm_phases.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                           ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)]
        L.kgs_bench_ntt.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                    ctypes.POINTER(ctypes.c_double)]
        L.kgs_verify.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_u8p, c_u8p, c_u8p]
        L.kgs_verify_ptau.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_u8p,
                                      c_u8p]
        L.kgs_verify_batch.argtypes = [ctypes.c_void_p, ctypes.POINTER(ProofRef), ctypes.c_int, c_u8p, c_u8p,
                                       ctypes.POINTER(BatchDiag)]
        L.kgs_verify_batch_ptau.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ProofRef), ctypes.c_int,
                                            c_u8p, ctypes.POINTER(BatchDiag)]
        L.kgs_multi_proof_shape.argtypes = [ctypes.POINTER(ArgShape), ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                            ctypes.POINTER(ctypes.c_int)]
        L.kgs_prove_multi.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Arg), ctypes.c_int, c_u8p, c_u8p]
        L.kgs_prove_multi_device.argtypes = L.kgs_prove_multi.argtypes
        L.kgs_verify_multi.argtypes = [ctypes.c_int, ctypes.POINTER(ArgShape), ctypes.c_int, c_u8p, c_u8p, c_u8p]
        L.kgs_verify_multi_ptau.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ArgShape), ctypes.c_int, c_u8p,
                                            c_u8p]
        L.kgs_g1_lincomb.argtypes = [ctypes.c_void_p, c_u8p, c_u8p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint64,
                                     c_u8p]
        L.kgs_msm_points.argtypes = [ctypes.c_void_p, c_u8p, c_u8p, ctypes.c_uint64, ctypes.c_int, c_u8p]
        L.kgs_msm_points_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                            ctypes.c_int, c_u8p]
        L.kgs_g1_ntt.argtypes = [ctypes.c_void_p, c_u8p, c_u8p, ctypes.c_int, ctypes.c_int]
        L.kgs_g1_ntt_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        L.kgs_srs_lagrange.argtypes = [ctypes.c_void_p, ctypes.c_int, c_u8p]
        L.kgs_commit_evals.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_int, c_u8p]
        L.kgs_commit_evals_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, c_u8p]
        L.kgs_g1_mul_each.argtypes = [ctypes.c_void_p, c_u8p, c_u8p, ctypes.c_uint64, c_u8p]
        L.kgs_g1_mul_each_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                             ctypes.c_void_p]
        L.kgs_kzg_open.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, c_u8p, c_u8p, c_u8p]
        L.kgs_kzg_open_all.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, ctypes.c_int, c_u8p, c_u8p]
        L.kgs_kzg_open_all_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                              ctypes.c_void_p, ctypes.c_void_p]
        L.kgs_kzg_verify.argtypes = [c_u8p, c_u8p, c_u8p, c_u8p, c_u8p]
        L.kgs_g1_mul_sum.argtypes = [ctypes.c_void_p, c_u8p, c_u8p, ctypes.c_uint64, ctypes.c_uint64, c_u8p]
        L.kgs_g1_mul_sum_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                            ctypes.c_uint64, ctypes.c_void_p]
        L.kgs_kzg_open_cosets.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, c_u8p,
                                          c_u8p]
        L.kgs_kzg_open_cosets_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                                 ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        L.kgs_kzg_open_cosets_cached.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        L.kgs_kzg_open_cosets_many.argtypes = [ctypes.c_void_p, c_u8p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                               ctypes.c_int, ctypes.c_int, c_u8p, c_u8p]
        L.kgs_kzg_open_cosets_many_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                                      ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                      ctypes.c_void_p]
        L.kgs_bench_kzg_open_cosets_many.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                                     ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                     ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
        L.kgs_kzg_verify_coset.argtypes = [c_u8p, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, c_u8p, c_u8p, c_u8p,
                                           c_u8p]
        L.kgs_kzg_verify_cosets_batch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, c_u8p, ctypes.c_uint64,
                                                  ctypes.c_void_p, ctypes.c_void_p, c_u8p, c_u8p, ctypes.c_uint64, c_u8p,
                                                  c_u8p, c_u8p, c_u8p, ctypes.POINTER(CosetBatchDiag)]
        L.kgs_kzg_verify_cosets_batch_device.argtypes = L.kgs_kzg_verify_cosets_batch.argtypes
        L.kgs_coset_interp_fold.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, c_u8p, c_u8p,
                                            ctypes.c_uint64, c_u8p]
        L.kgs_coset_interp_fold_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        L.kgs_kzg_recover_cosets.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, c_u8p,
                                             ctypes.c_uint64, ctypes.c_uint64, c_u8p, c_u8p]
        L.kgs_kzg_recover_cosets_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                    ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                                                    ctypes.c_void_p]
        L.kgs_bench_kzg_recover_cosets.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                   ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                                                   ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                   ctypes.POINTER(ctypes.c_double)]
        L.kgs_kzg_recover_cosets_many.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint64,
                                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                  ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, c_u8p, c_u8p]
        L.kgs_kzg_recover_cosets_many_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint64,
                                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                         ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                                         ctypes.c_void_p, ctypes.c_void_p, c_u8p]
        L.kgs_bench_kzg_recover_cosets_many.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint64,
                                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                        ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                                        ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                        ctypes.POINTER(ctypes.c_double)]
        L.kgs_ptau_read_tau_g2_pow.argtypes = [ctypes.c_char_p, ctypes.c_uint64, c_u8p]
        L.kgs_ctx_set_shard.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        L.kgs_ctx_set_msm_lanes.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.kgs_ctx_set_reference_quirks.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.kgs_shard_range.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64),
                                      ctypes.POINTER(ctypes.c_uint64)]
        L.kgs_msm_combine.argtypes = [c_u8p, ctypes.c_int, ctypes.c_int, c_u8p]
        L.kgs_group_create_local.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        L.kgs_group_create_host.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.POINTER(ctypes.c_void_p)]
        L.kgs_group_create_host_a2a.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.POINTER(ctypes.c_void_p)]
        L.kgs_last_exchange.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int]
        L.kgs_group_rccl_unique_id.argtypes = [c_u8p]
        L.kgs_group_create_rccl.argtypes = [ctypes.c_int, ctypes.c_int, c_u8p, ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_void_p)]
        L.kgs_group_destroy.argtypes = [ctypes.c_void_p]
        L.kgs_group_destroy.restype = None
        L.kgs_group_world.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
        L.kgs_ctx_set_group.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        _lib = L
    return _lib


# int (*kgs_allgather_fn)(void* user, const uint8_t* send, uint8_t* recv, uint64_t bytes)
ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64)
# int (*kgs_alltoall_fn)(void* user, const uint8_t* send, uint8_t* recv, uint64_t chunk)
ALLTOALL_FN = ALLGATHER_FN


def _check(rc):
    if rc < 0:
        raise KgsError(rc, lib().kgs_last_error().decode())
    return rc


def _buf(b):
    """bytes-like -> (ctypes buffer, pointer) keeping it alive."""
    cb = ctypes.create_string_buffer(bytes(b), len(b)) if b is not None else None
    return cb


_PBA = ctypes.pythonapi.PyByteArray_FromStringAndSize
_PBA.restype = ctypes.py_object
_PBA.argtypes = [ctypes.c_char_p, ctypes.c_ssize_t]


def _uninit_bytearray(n):
    """bytearray of n bytes WITHOUT the zero fill of bytearray(n) (CPython C API; the library
    overwrites every byte): saves a 32 MiB memset per written-back vector at n = 2^20."""
    return _PBA(None, n)


def _ptr(b):
    """Zero-copy pointer to a bytes-like object's memory: (pointer, keep-alive). bytes are read
    in place (c_char_p); writable buffers (bytearray, numpy) through from_buffer; anything else
    is copied once."""
    if isinstance(b, bytes):
        cp = ctypes.c_char_p(b)
        return ctypes.cast(cp, ctypes.c_void_p), (b, cp)
    try:
        arr = (ctypes.c_char * len(b)).from_buffer(b)
        return ctypes.cast(arr, ctypes.c_void_p), (b, arr)
    except (TypeError, ValueError):
        cb = ctypes.create_string_buffer(bytes(b), len(b))
        return ctypes.cast(cb, ctypes.c_void_p), cb


def keccak256(data: bytes) -> bytes:
    out = ctypes.create_string_buffer(32)
    src = ctypes.create_string_buffer(bytes(data), max(1, len(data)))
    _check(lib().kgs_keccak256(src, len(data), out))
    return out.raw


def ptau_power(path):
    """Power of a ptau file, from its header only (kgs_ptau_power; readPTauHeader, ptau_utils.js:3-24)."""
    p = ctypes.c_int()
    _check(lib().kgs_ptau_power(os.fsencode(path), ctypes.byref(p)))
    return p.value


def device_count():
    n = ctypes.c_int()
    _check(lib().kgs_device_count(ctypes.byref(n)))
    return n.value


def host_register(buf):
    """Pin a writable host buffer (bytearray / numpy) that several proofs will reuse: kgs_prove then
    DMAs it in place instead of through pinned staging (kgs_host_register). Returns a handle to pass
    to host_unregister before the buffer is released or resized."""
    p, keep = _ptr(buf)
    if isinstance(keep, ctypes.Array):
        raise TypeError("host_register needs a writable buffer (bytearray, numpy array)")
    _check(lib().kgs_host_register(p, len(buf)))
    return p, keep


def host_unregister(handle):
    _check(lib().kgs_host_unregister(handle[0]))


def shard_range(n, rank, world):
    """Point range [lo, hi) of an n-point MSM owned by `rank` (kgs_shard_range)."""
    lo, hi = ctypes.c_uint64(), ctypes.c_uint64()
    _check(lib().kgs_shard_range(n, rank, world, ctypes.byref(lo), ctypes.byref(hi)))
    return lo.value, hi.value


def msm_combine(T_all, nparts, c):
    """Commitment (64 B affine LEM) from `nparts` rank partials of c XYZZ bit-sum points each."""
    if len(T_all) != nparts * c * 128:
        raise ValueError("T_all must hold nparts * c * 128 bytes")
    out = ctypes.create_string_buffer(64)
    _check(lib().kgs_msm_combine(_buf(T_all), nparts, c, out))
    return out.raw


def torch_allgather(group=None, device=None):
    """All-gather transport for Context.set_shard over torch.distributed: RCCL (backend "nccl")
    when `device` is a GPU, gloo on host tensors otherwise."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)

    def fn(data):
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8)
        if device is not None:
            t = t.to(device)
        outs = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(outs, t, group=group)
        return b"".join(o.cpu().numpy().tobytes() for o in outs)
    return fn


def torch_alltoall(group=None):
    """All-to-all transport for Group.host over torch.distributed (all_to_all_single on host tensors:
    gloo): alltoall(data, chunk) sends chunk j of `data` to rank j and returns the world chunks
    received, rank-major."""
    import torch
    import torch.distributed as dist

    def fn(data, chunk):
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8)
        out = torch.empty_like(t)
        dist.all_to_all_single(out, t, group=group)
        return out.numpy().tobytes()
    return fn


class Group:
    """Rank group of the distributed prover (kgs_group_t; Context.set_group): every vector of a
    proof sharded over `world` ranks, one context per rank.
      Group.local(world)                 several contexts of this process (one host thread per rank)
      Group.host(world, allgather[, alltoall])
                                         any host all-gather(bytes) -> world * bytes (e.g. gloo) and,
                                         optionally, an all-to-all(bytes, chunk) -> bytes (chunk j to
                                         rank j: (W - 1) / W of a vector leaves a rank instead of every
                                         rank receiving W x it); device data is staged through the host
      Group.rccl(rank, world, id, dev)   one process per GPU, RCCL over xGMI; id = rccl_unique_id()
                                         made on rank 0 and broadcast by the caller"""

    def __init__(self, handle, world, keep=None):
        self._h = handle
        self.world = world
        self._keep = keep

    @classmethod
    def local(cls, world):
        h = ctypes.c_void_p()
        _check(lib().kgs_group_create_local(world, ctypes.byref(h)))
        return cls(h, world)

    @classmethod
    def host(cls, world, allgather, alltoall=None):
        def _cb(user, send, recv, nbytes):
            try:
                out = allgather(ctypes.string_at(send, nbytes))
                if len(out) != nbytes * world:
                    return -1
                ctypes.memmove(recv, out, len(out))
                return 0
            except Exception:  # reported to the caller as KGS_E_COMM
                import traceback
                traceback.print_exc()
                return -1

        def _a2a(user, send, recv, chunk):
            try:
                out = alltoall(ctypes.string_at(send, chunk * world), chunk)
                if len(out) != chunk * world:
                    return -1
                ctypes.memmove(recv, out, len(out))
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                return -1
        cb = ALLGATHER_FN(_cb)
        h = ctypes.c_void_p()
        if alltoall is None:
            _check(lib().kgs_group_create_host(world, ctypes.cast(cb, ctypes.c_void_p), None, ctypes.byref(h)))
            return cls(h, world, cb)
        cb2 = ALLTOALL_FN(_a2a)
        _check(lib().kgs_group_create_host_a2a(world, ctypes.cast(cb, ctypes.c_void_p), ctypes.cast(cb2, ctypes.c_void_p),
                                               None, ctypes.byref(h)))
        return cls(h, world, (cb, cb2))

    @classmethod
    def rccl(cls, rank, world, uid, device):
        h = ctypes.c_void_p()
        _check(lib().kgs_group_create_rccl(rank, world, _buf(uid), device, ctypes.byref(h)))
        return cls(h, world)

    def close(self):
        if self._h:
            lib().kgs_group_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rccl_unique_id():
    """128-byte RCCL communicator id (kgs_group_rccl_unique_id), made on rank 0 and broadcast."""
    out = ctypes.create_string_buffer(128)
    _check(lib().kgs_group_rccl_unique_id(out))
    return out.raw


class ThreadGroup:
    """In-process all-gather between `world` contexts driven by `world` host threads (one rank
    each): several GPUs of one process, or the sharded path rehearsed on a single GPU."""

    def __init__(self, world):
        import threading
        self.world = world
        self._bar = threading.Barrier(world)
        self._slots = [None] * world

    def allgather(self, rank):
        def fn(data):
            self._slots[rank] = bytes(data)
            self._bar.wait()
            out = b"".join(self._slots)
            self._bar.wait()
            return out
        return fn


class Evaluations:
    """Mirror of src/polynomial/evaluations.js (the prover's input container): `.eval` bytes."""

    def __init__(self, eval_bytes):
        self.eval = bytes(eval_bytes)

    def length(self):
        if len(self.eval) % 32:
            raise ValueError("Polynomial evaluations buffer has incorrect size")
        return len(self.eval) // 32

    @staticmethod
    def getOneEvals(length):
        return Evaluations(FR_ONE_MONT * length)

    def isAllOnes(self):
        return self.eval == FR_ONE_MONT * self.length()

    def isAllZeros(self):
        return self.eval == bytes(len(self.eval))


class Context:
    """One HIP device + resident SRS. Not re-entrant (like the reference's curve object)."""

    def __init__(self, device=0):
        self._h = ctypes.c_void_p()
        _check(lib().kgs_ctx_create(device, ctypes.byref(self._h)))
        self._srs = None

    def close(self):
        if self._h:
            lib().kgs_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def set_reference_quirks(self, on):
        """Reference-quirks mode (kgs_ctx_set_reference_quirks; default ON unless the environment has
        KGS_REFERENCE_QUIRKS == "0"): reproduce the reference's failures on degenerate inputs; off, the
        exact-math prover proves them."""
        _check(lib().kgs_ctx_set_reference_quirks(self._h, 1 if on else 0))

    def set_msm_lanes(self, lanes):
        """1 or 2 HIP streams for the independent MSMs of a prover round (kgs_ctx_set_msm_lanes)."""
        _check(lib().kgs_ctx_set_msm_lanes(self._h, lanes))

    def set_shard(self, rank, world, allgather=None):
        """MSM point-range sharding (kgs_ctx_set_shard): `allgather(bytes) -> world * bytes`
        (rank-major), called in the same order on every rank. world == 1 switches it off."""
        if world > 1 and allgather is None:
            raise ValueError("sharding needs an all-gather transport")

        def _cb(user, send, recv, nbytes):
            try:
                out = allgather(ctypes.string_at(send, nbytes))
                if len(out) != nbytes * world:
                    return -1
                ctypes.memmove(recv, out, len(out))
                return 0
            except Exception:  # reported to the caller as KGS_E_COMM
                import traceback
                traceback.print_exc()
                return -1
        self._shard_cb = ALLGATHER_FN(_cb) if world > 1 else None
        fp = ctypes.cast(self._shard_cb, ctypes.c_void_p) if world > 1 else None
        _check(lib().kgs_ctx_set_shard(self._h, rank, world, fp, None))

    def set_group(self, group, rank=0):
        """Attach the distributed prover (kgs_ctx_set_group): this context is `rank` of `group`;
        None detaches. Keeps the group alive while attached."""
        _check(lib().kgs_ctx_set_group(self._h, group._h if group is not None else None, rank))
        self._group = group

    def load_ptau(self, path, nbits_max=-1, slice=None):
        """kgs_srs_load_ptau; slice=(rank, world): only rank's slice of the SRS, the points rank + world*j
        (kgs_srs_load_ptau_slice) — what a rank of the distributed prover commits with"""
        if slice is None:
            _check(lib().kgs_srs_load_ptau(self._h, os.fsencode(path), nbits_max))
        else:
            _check(lib().kgs_srs_load_ptau_slice(self._h, os.fsencode(path), nbits_max, int(slice[0]), int(slice[1])))
        self._srs = (path, nbits_max, slice)

    def srs_slice_info(self):
        """(rank, world, window-table bytes) of the resident SRS (world 1: the whole prefix)"""
        r, w, b = ctypes.c_int(), ctypes.c_int(), ctypes.c_uint64()
        _check(lib().kgs_srs_slice_info(self._h, ctypes.byref(r), ctypes.byref(w), ctypes.byref(b)))
        return r.value, w.value, b.value

    def srs_info(self):
        p, c = ctypes.c_int(), ctypes.c_int()
        n = ctypes.c_uint64()
        _check(lib().kgs_srs_info(self._h, ctypes.byref(p), ctypes.byref(n), ctypes.byref(c)))
        return p.value, n.value, c.value

    def write_synthetic_ptau(self, path, power, tau):
        t = ctypes.create_string_buffer(int(tau % R).to_bytes(32, "little"), 32)
        _check(lib().kgs_ptau_write_synthetic(self._h, os.fsencode(path), power, t))

    # ---- primitives (host buffers) ----
    def fr_to_mont(self, data):
        n = len(data) // 32
        out = ctypes.create_string_buffer(32 * n)
        _check(lib().kgs_fr_to_mont(self._h, _buf(data), out, n))
        return out.raw

    def fr_from_mont(self, data):
        n = len(data) // 32
        out = ctypes.create_string_buffer(32 * n)
        _check(lib().kgs_fr_from_mont(self._h, _buf(data), out, n))
        return out.raw

    def fr_batch_inverse(self, data):
        n = len(data) // 32
        out = ctypes.create_string_buffer(32 * n)
        _check(lib().kgs_fr_batch_inverse(self._h, _buf(data), out, n))
        return out.raw

    def ntt(self, data, inverse=False):
        m = len(data) // 32
        logm = m.bit_length() - 1
        out = ctypes.create_string_buffer(32 * m)
        _check(lib().kgs_ntt(self._h, _buf(data), out, logm, 1 if inverse else 0))
        return out.raw

    def ntt_ex(self, data, logm, flags=0):
        """kgs_ntt_ex: the transforms as the provers launch them. data holds in_len = len(data) / 32
        elements (forward: 0 .. 2^logm; inverse: 2^logm), flags is an OR of NTT_*; the result has
        2^logm elements. include/kgs.h states each combination as a formula."""
        in_len = len(data) // 32
        if flags & NTT_INVERSE and 0 <= logm <= 28 and in_len != 1 << logm:
            raise ValueError("an inverse transform takes 2^logm elements")
        out = ctypes.create_string_buffer(32 << logm if 0 <= logm <= 28 else 32)
        _check(lib().kgs_ntt_ex(self._h, _buf(data) if in_len else None, in_len, out, logm, flags))
        return out.raw

    def ntt_blocks(self, data, logtotal, s, flags=0):
        """kgs_ntt_blocks: the 2^(logtotal - s) transforms of size 2^s over the consecutive blocks of data
        (2^logtotal elements) as the coset openings and the recovery launch them. Forward: every block natural
        in, bit-reversed out; NTT_INVERSE: bit-reversed in, natural out, with 1/2^s unless NTT_NO_SCALE;
        NTT_INFLIGHT: the other pass build. include/kgs.h states the result as a formula."""
        in_range = 0 <= logtotal <= 28  # else the library refuses before it reads
        if in_range and len(data) != 32 << logtotal:
            raise ValueError("the block transforms take 2^logtotal elements")
        out = ctypes.create_string_buffer(32 << logtotal if in_range else 32)
        _check(lib().kgs_ntt_blocks(self._h, _buf(data), out, logtotal, s, flags))
        return out.raw

    def msm(self, scalars_mont):
        n = len(scalars_mont) // 32
        out = ctypes.create_string_buffer(64)
        _check(lib().kgs_msm(self._h, _buf(scalars_mont) if n else None, n, out))
        return out.raw

    def grand_build(self, kind, f_mont, t_mont, gamma_mont, sel_f=None, sel_t=None):
        n = len(f_mont) // 32
        out = ctypes.create_string_buffer(32 * n)
        _check(lib().kgs_grand_build(self._h, kind, _buf(f_mont), _buf(t_mont), _buf(sel_f), _buf(sel_t),
                                     _buf(gamma_mont), n, out))
        return out.raw

    def quotient_ex(self, nbits, lcs, args, alpha_mont, gamma_mont, delta_mont=None, flags=0):
        """kgs_quotient_ex: round 3's quotient launches on a coset of 2^lcs points. args is a list of
        (kind, S, F, T, sel_f, sel_t): Montgomery buffers of 2^lcs elements in the kernels' (bit-reversed)
        order, sel_f / sel_t None for an unselected argument. Returns q as 2^lcs elements; include/kgs.h
        states it as a formula."""
        shape_ok = 1 <= nbits <= 27 and lcs in (nbits, nbits + 1)  # else the library refuses before it reads
        cs = 1 << lcs if shape_ok else 1
        recs = (QuotArg * max(len(args), 1))()
        keep = []
        for j, (kind, *bufs) in enumerate(args):
            ptrs = []
            for b in bufs:
                if shape_ok and b is not None and len(b) != 32 * cs:
                    raise ValueError("every array holds 2^lcs 32-byte elements")
                p, k = _ptr(b) if b is not None else (None, None)
                ptrs.append(p)
                keep.append(k)
            recs[j] = QuotArg(kind, *ptrs)
        out = ctypes.create_string_buffer(32 * cs)
        _check(lib().kgs_quotient_ex(self._h, nbits, lcs, recs, len(args), _buf(alpha_mont), _buf(gamma_mont),
                                     _buf(delta_mont), flags, out))
        return out.raw

    def divcheck(self, kind, S, f, t, alpha_mont, gamma_mont, sel_f=None, sel_t=None, s_next=None, gbase=0):
        """kgs_divcheck: round 3's divisibility check over n = len(S) / 32 natural-order elements (any n);
        s_next is S past the last element (None: S[0]), gbase the natural index of element 0. Returns 1
        if the numerator is nonzero somewhere, else 0."""
        n = len(S) // 32
        if any(b is not None and len(b) != 32 * n for b in (f, t, sel_f, sel_t)):
            raise ValueError("every array holds as many elements as S")
        nz = ctypes.c_int(-1)
        _check(lib().kgs_divcheck(self._h, kind, n, _buf(S), _buf(f), _buf(t), _buf(sel_f), _buf(sel_t), _buf(alpha_mont),
                                  _buf(gamma_mont), _buf(s_next), gbase, ctypes.byref(nz)))
        return nz.value

    def lincomb(self, srcs, coefs_mont, c0_mont, out_len, lens=None):
        """kgs_lincomb: out[i] = sum_k coef_k srcs[k][i] (i < lens[k]) + (i == 0 ? c0 : 0) through the
        provers' run_lincomb. srcs: Montgomery buffers (the same object given twice is one buffer);
        lens: elements of each (default: all of it); coefs_mont: len(srcs) x 32 B. Returns out_len elements."""
        count = len(srcs)
        lens = [len(s) // 32 for s in srcs] if lens is None else list(lens)
        if len(lens) != count or len(coefs_mont) != 32 * count or any(32 * l > len(s) for s, l in zip(srcs, lens)):
            raise ValueError("one length and one coefficient per source, no length beyond its buffer")
        P = (ctypes.c_void_p * max(count, 1))()
        seen = {}
        for k, s in enumerate(srcs):
            if id(s) not in seen:
                seen[id(s)] = _ptr(s) if len(s) else (None, None)
            P[k] = seen[id(s)][0]
        L = (ctypes.c_uint64 * max(count, 1))(*lens)
        out = ctypes.create_string_buffer(32 * out_len if 1 <= out_len <= 1 << 28 else 32)
        _check(lib().kgs_lincomb(self._h, P, L, _buf(coefs_mont), count, _buf(c0_mont), out_len, out))
        return out.raw

    def poly_eval(self, coef_mont, x_mont):
        out = ctypes.create_string_buffer(32)
        _check(lib().kgs_poly_eval(self._h, _buf(coef_mont), len(coef_mont) // 32, _buf(x_mont), out))
        return out.raw

    def poly_div_x_sub(self, coef_mont, z_mont):
        out = ctypes.create_string_buffer(len(coef_mont))
        _check(lib().kgs_poly_div_x_sub(self._h, _buf(coef_mont), len(coef_mont) // 32, _buf(z_mont), out))
        return out.raw

    def lookup_multiplicities(self, evals_f, evals_t, sel_f=None):
        """Multiplicities of the table rows of a lookup (kgs_lookup_multiplicities): evals_f / evals_t are
        lists of k standard-form buffers of n 32-byte elements (any n >= 1), sel_f a Montgomery selector
        or None (every row selected). Returns n Montgomery elements as a bytearray: the evalsMulT of
        lookup_prover. A repeated table row gets all of its count at its first occurrence. Inputs are
        read in place and left as they are."""
        k = len(evals_f)
        if k == 0 or len(evals_t) != k:
            raise ValueError("evals_f and evals_t must be two lists of the same, nonzero number of columns")
        nbytes = len(evals_f[0])
        bufs = list(evals_f) + list(evals_t) + ([sel_f] if sel_f is not None else [])
        if nbytes == 0 or nbytes % 32 or any(len(x) != nbytes for x in bufs):
            raise ValueError("every buffer must hold the same number (>= 1) of 32-byte elements")
        keep = []
        PF = (ctypes.c_void_p * k)()
        PT = (ctypes.c_void_p * k)()
        for i in range(k):
            (pf, kf), (pt, kt) = _ptr(evals_f[i]), _ptr(evals_t[i])
            keep += [kf, kt]
            PF[i], PT[i] = pf, pt
        sf = None
        if sel_f is not None:
            sf, ksf = _ptr(sel_f)
            keep.append(ksf)
        out = _uninit_bytearray(nbytes)
        po, ko = _ptr(out)
        keep.append(ko)
        _check(lib().kgs_lookup_multiplicities(self._h, k, nbytes // 32, PF, PT, sf, po))
        return out

    def lookup_multiplicities_device(self, d_f, d_t, d_sf, d_out, n):
        """Device-resident twin (kgs_lookup_multiplicities_device): d_f / d_t are lists of device pointers
        (ints) to n standard-form elements, d_sf a device pointer to the Montgomery selector or None,
        d_out a device pointer to n x 32 writable bytes — afterwards the d_st of
        prove_device(LOOKUP, ..)."""
        k = len(d_f)
        PF = (ctypes.c_void_p * k)(*d_f)
        PT = (ctypes.c_void_p * k)(*d_t)
        _check(lib().kgs_lookup_multiplicities_device(self._h, k, n, PF, PT, d_sf, d_out))

    def verify_batch(self, items, tau_g2=None, ptau=None, locate=True, diag=None):
        """Batch verifier (kgs_verify_batch) with the fold on this context's GPU: see the module-level
        verify_batch. Exactly one of tau_g2 (128 B LEM) and ptau (a file name) is given."""
        return _verify_batch(self._h, items, tau_g2, ptau, locate, diag)

    def g1_lincomb(self, points_lem, scalars_std, seg_off):
        """Segmented G1 linear combination on the GPU (kgs_g1_lincomb): see the module-level g1_lincomb."""
        return _g1_lincomb(self._h, points_lem, scalars_std, seg_off)

    def msm_points(self, points_lem, scalars_std, window_c=0):
        """Variable-base MSM on the GPU (kgs_msm_points): see the module-level msm_points."""
        return _msm_points(self._h, points_lem, scalars_std, window_c)

    def msm_points_device(self, d_points, d_scalars, n, window_c=0):
        """Device-resident twin (kgs_msm_points_device): d_points / d_scalars are device pointers (ints)
        to n affine LEM points of 64 B and n standard-form scalars of 32 B, both read only. Returns the
        64 B affine LEM sum."""
        out = ctypes.create_string_buffer(64)
        _check(lib().kgs_msm_points_device(self._h, d_points, d_scalars, n, window_c, out))
        return out.raw

    def g1_ntt(self, points_lem, inverse=False):
        """G1.fft / G1.ifft on the GPU (kgs_g1_ntt): see the module-level g1_ntt."""
        return _g1_ntt(self._h, points_lem, inverse)

    def g1_ntt_device(self, d_in, d_out, logm, inverse=False):
        """Device-resident twin (kgs_g1_ntt_device): d_in / d_out are device pointers (ints) to 2^logm
        affine LEM points of 64 B; d_in is only read unless d_out is the same pointer, which is allowed."""
        _check(lib().kgs_g1_ntt_device(self._h, d_in, d_out, logm, 1 if inverse else 0))

    def srs_lagrange(self, nbits, fetch=True):
        """The Lagrange-basis SRS [L_i(tau)]_1, i < 2^nbits, of the resident SRS (kgs_srs_lagrange), built
        on the GPU on first use and cached on the device per (SRS, nbits). Returns 2^nbits x 64 B affine
        LEM; fetch=False only builds and caches, and returns None."""
        if not fetch:
            _check(lib().kgs_srs_lagrange(self._h, nbits, None))
            return None
        out = ctypes.create_string_buffer(64 << nbits if 0 <= nbits <= 24 else 64)
        _check(lib().kgs_srs_lagrange(self._h, nbits, out))
        return out.raw

    def commit_evals(self, evals_std, nbits=None):
        """Commitment from evaluations (kgs_commit_evals): sum_i e_i [L_i(tau)]_1 over the resident SRS, the
        bytes msm(ntt(fr_to_mont(e), inverse=True)) gives, without the coefficients. evals_std: 2^nbits
        standard-form elements of 32 B, any 256-bit integers (nbits=None: from the length). Returns 64 B
        affine LEM (zeros for the identity)."""
        m = len(evals_std) // 32
        if nbits is None:
            nbits = m.bit_length() - 1
        if len(evals_std) % 32 or not 0 <= nbits <= 24 or m != 1 << nbits:
            raise ValueError("evals_std must hold 2^nbits 32-byte elements, nbits in 0 .. 24")
        out = ctypes.create_string_buffer(64)
        pe, ke = _ptr(evals_std)  # read in place
        _check(lib().kgs_commit_evals(self._h, pe, nbits, out))
        del ke
        return out.raw

    def commit_evals_device(self, d_evals, nbits):
        """Device-resident twin (kgs_commit_evals_device): d_evals is a device pointer (int) to 2^nbits
        standard-form elements, read only."""
        out = ctypes.create_string_buffer(64)
        _check(lib().kgs_commit_evals_device(self._h, d_evals, nbits, out))
        return out.raw

    def g1_mul_each(self, points_lem, scalars_std):
        """One scalar per point on the GPU (kgs_g1_mul_each): see the module-level g1_mul_each."""
        return _g1_mul_each(self._h, points_lem, scalars_std)

    def g1_mul_each_device(self, d_points, d_scalars, n, d_out):
        """Device-resident twin (kgs_g1_mul_each_device): device pointers (ints) to n affine LEM points of
        64 B, n standard-form scalars of 32 B and n x 64 writable bytes, which may be the points' own."""
        _check(lib().kgs_g1_mul_each_device(self._h, d_points, d_scalars, n, d_out))

    def kzg_open(self, coef_mont, z_mont):
        """One KZG opening over the resident SRS (kgs_kzg_open): coef_mont holds the polynomial's Montgomery
        coefficients (32 B each, any number the SRS covers), z_mont the point. Returns (y, proof):
        y = p(z) as 32 B Montgomery and [(p(X) - y) / (X - z)](tau) as 64 B affine LEM."""
        if len(coef_mont) % 32 or len(z_mont) != 32:
            raise ValueError("coef_mont must hold 32-byte elements and z_mont one of them")
        y, proof = ctypes.create_string_buffer(32), ctypes.create_string_buffer(64)
        n = len(coef_mont) // 32
        pc, kc = _ptr(coef_mont) if n else (None, None)  # read in place
        _check(lib().kgs_kzg_open(self._h, pc, n, _buf(z_mont), y, proof))
        del kc
        return y.raw, proof.raw

    def kzg_open_all(self, coef_mont, nbits=None, evals=False):
        """All 2^nbits openings of a polynomial on its domain in O(n log n) (kgs_kzg_open_all, FK20): entry i
        of the result is the proof kzg_open gives at Fr.w[nbits]^i, byte for byte. coef_mont: at most
        2^nbits Montgomery coefficients of 32 B (nbits=None: the smallest domain that holds them). The SRS
        side of the product is built on first use and cached on the device per (SRS, nbits). Returns
        2^nbits x 64 B affine LEM, or with evals=True the pair (proofs, p(w^i) as 2^nbits x 32 B Montgomery)."""
        n = len(coef_mont) // 32
        if nbits is None:
            nbits = max(n - 1, 0).bit_length()
        if len(coef_mont) % 32:
            raise ValueError("coef_mont must hold 32-byte elements")
        m = 1 << nbits if 0 <= nbits <= 23 else 1  # else the library refuses before it writes
        proofs = ctypes.create_string_buffer(64 * m)
        ev = ctypes.create_string_buffer(32 * m) if evals else None
        pc, kc = _ptr(coef_mont) if n else (None, None)  # read in place
        _check(lib().kgs_kzg_open_all(self._h, pc, n, nbits, proofs, ev))
        del kc
        return (proofs.raw, ev.raw) if evals else proofs.raw

    def kzg_open_all_device(self, d_coef, n, nbits, d_proofs, d_evals=None):
        """Device-resident twin (kgs_kzg_open_all_device): d_coef is a device pointer (int) to n <= 2^nbits
        Montgomery coefficients, read only; d_proofs to 2^nbits x 64 writable bytes; d_evals to 2^nbits x
        32 writable bytes, or None."""
        _check(lib().kgs_kzg_open_all_device(self._h, d_coef, n, nbits, d_proofs, d_evals))

    def g1_mul_sum(self, points_lem, scalars_std, rows):
        """Column sums of per-point products on the GPU (kgs_g1_mul_sum): see the module-level g1_mul_sum."""
        return _g1_mul_sum(self._h, points_lem, scalars_std, rows)

    def g1_mul_sum_device(self, d_points, d_scalars, rows, cols, d_out):
        """Device-resident twin (kgs_g1_mul_sum_device): device pointers (ints) to rows * cols affine LEM
        points of 64 B and as many standard-form scalars of 32 B, both only read, and cols x 64 writable bytes."""
        _check(lib().kgs_g1_mul_sum_device(self._h, d_points, d_scalars, rows, cols, d_out))

    def kzg_open_cosets(self, coef_mont, nbits, lbits, evals=False):
        """Every coset opening of a polynomial at once (kgs_kzg_open_cosets): with n = 2^nbits, l = 2^lbits
        and m = n / l, entry i < m of the result is the one 64 B proof for the l values p(w^(i + m j)), j < l,
        on the coset w^i <w^m> (w = Fr.w[nbits]). coef_mont: at most 2^nbits Montgomery coefficients of
        32 B. lbits = 0 is kzg_open_all. The SRS side is built on first use and cached on the device per (SRS,
        nbits, lbits). Returns m x 64 B affine LEM, or with evals=True the pair (proofs, p(w^k) in natural
        order as 2^nbits x 32 B Montgomery)."""
        if len(coef_mont) % 32:
            raise ValueError("coef_mont must hold 32-byte elements")
        n = len(coef_mont) // 32
        ok = 0 <= nbits <= 23 and 0 <= lbits <= nbits  # else the library refuses before it writes
        proofs = ctypes.create_string_buffer(64 << (nbits - lbits) if ok else 64)
        ev = ctypes.create_string_buffer(32 << nbits if ok else 32) if evals else None
        pc, kc = _ptr(coef_mont) if n else (None, None)  # read in place
        _check(lib().kgs_kzg_open_cosets(self._h, pc, n, nbits, lbits, proofs, ev))
        del kc
        return (proofs.raw, ev.raw) if evals else proofs.raw

    def kzg_open_cosets_cached(self, nbits, lbits):
        """True when the SRS side for (nbits, lbits) is cached on the device (kgs_kzg_open_cosets_cached): a
        call with these sizes builds nothing. lbits = 0 asks for kzg_open_all's row."""
        return _check(lib().kgs_kzg_open_cosets_cached(self._h, nbits, lbits)) == 1

    def kzg_open_cosets_device(self, d_coef, n, nbits, lbits, d_proofs, d_evals=None):
        """Device-resident twin (kgs_kzg_open_cosets_device): d_coef is a device pointer (int) to n <= 2^nbits
        Montgomery coefficients, read only; d_proofs to 2^(nbits - lbits) x 64 writable bytes; d_evals to
        2^nbits x 32 writable bytes, or None."""
        _check(lib().kgs_kzg_open_cosets_device(self._h, d_coef, n, nbits, lbits, d_proofs, d_evals))

    def kzg_open_cosets_many(self, coefs, nbits, lbits, evals=False):
        """kzg_open_cosets for many polynomials over one (nbits, lbits) in one call (kgs_kzg_open_cosets_many): every
        stage runs once for the whole set, so small polynomials share the latency a single call pays alone. coefs:
        a list of bytes-likes of Montgomery coefficients, at most 2^nbits of 32 B each; unequal lengths are
        zero-padded to the longest, which changes no proof. len(coefs) * 2^nbits is at most 2^24. Returns the list
        of the proofs kzg_open_cosets gives for each polynomial, byte for byte, or with evals=True the pair (list
        of proofs, list of evaluations)."""
        coefs = [bytes(c) for c in coefs]
        if any(len(c) % 32 for c in coefs):
            raise ValueError("coefs must hold 32-byte elements")
        polys = len(coefs)
        n = max((len(c) // 32 for c in coefs), default=0)
        packed = b"".join(c + bytes(32 * n - len(c)) for c in coefs)
        ok = 0 <= nbits <= 23 and 0 <= lbits <= nbits  # else the library refuses before it writes
        psz, esz = (64 << (nbits - lbits), 32 << nbits) if ok else (64, 32)
        proofs = ctypes.create_string_buffer(max(psz * polys, 1))
        ev = ctypes.create_string_buffer(max(esz * polys, 1)) if evals else None
        pc, kc = _ptr(packed) if packed else (None, None)  # read in place
        _check(lib().kgs_kzg_open_cosets_many(self._h, pc, polys, n, n, nbits, lbits, proofs, ev))
        del kc
        out = [proofs.raw[psz * b:psz * (b + 1)] for b in range(polys)]
        return (out, [ev.raw[esz * b:esz * (b + 1)] for b in range(polys)]) if evals else out

    def kzg_open_cosets_many_device(self, d_coef, polys, stride, n, nbits, lbits, d_proofs, d_evals=None):
        """Device-resident twin (kgs_kzg_open_cosets_many_device): d_coef is a device pointer (int), read only,
        polynomial b's n <= 2^nbits Montgomery coefficients at d_coef + 32 * stride * b (stride >= n; the gap is
        not read); d_proofs to polys * 2^(nbits - lbits) x 64 writable bytes; d_evals to polys * 2^nbits x 32
        writable bytes, or None."""
        _check(lib().kgs_kzg_open_cosets_many_device(self._h, d_coef, polys, stride, n, nbits, lbits, d_proofs, d_evals))

    def kzg_verify_cosets_batch(self, tau_l_g2, srs_g1, nbits, lbits, commits, openings, locate=True, seed=None,
                                diag=None):
        """Batch verifier for coset openings (kgs_kzg_verify_cosets_batch) with the folds on this context's GPU:
        see the module-level kzg_verify_cosets_batch."""
        return _kzg_verify_cosets_batch(self._h, tau_l_g2, srs_g1, nbits, lbits, commits, openings, locate, seed, diag)

    def kzg_verify_cosets_batch_device(self, tau_l_g2, srs_g1, nbits, lbits, commits, d_commit_of, d_index, d_ys,
                                       d_proofs, count, seed, locate=True, diag=None):
        """Device-resident twin (kgs_kzg_verify_cosets_batch_device): d_commit_of (count x uint32), d_index (count x
        uint64), d_ys (count * 2^lbits x 32 B Montgomery) and d_proofs (count x 64 B) are device pointers (ints),
        only read; commits (a list of 64 B points, or their concatenation), srs_g1 and tau_l_g2 are host bytes.
        seed: 32 bytes, unpredictable to whoever made the proofs (required: nothing on the device is hashed).
        Returns a list of count bools, or one bool with locate=False."""
        if seed is None or len(seed) != 32:
            raise ValueError("the device twin needs a 32-byte seed")
        commits = _commit_bytes(commits)
        l = 1 << lbits if 0 <= lbits <= 28 else 0
        if len(srs_g1) < 64 * l:
            raise ValueError("srs_g1 must hold at least 2^lbits x 64 bytes")
        return _coset_batch_call(lib().kgs_kzg_verify_cosets_batch_device, self._h, tau_l_g2, srs_g1, nbits, lbits,
                                 commits, d_commit_of, d_index, d_ys, d_proofs, count, seed, locate, diag)

    def coset_interp_fold(self, nbits, lbits, index, ys_mont, weights_mont):
        """The weighted sum of interpolants on the GPU (kgs_coset_interp_fold): see the module-level
        coset_interp_fold."""
        return _coset_interp_fold(self._h, nbits, lbits, index, ys_mont, weights_mont)

    def coset_interp_fold_device(self, nbits, lbits, d_index, d_ys, d_weights, count, d_out):
        """Device-resident twin (kgs_coset_interp_fold_device): device pointers (ints) to count x uint64 indices,
        count * 2^lbits x 32 B values, count x 32 B weights, all only read, and 2^lbits x 32 writable bytes."""
        _check(lib().kgs_coset_interp_fold_device(self._h, nbits, lbits, d_index, d_ys, d_weights, count, d_out))

    def kzg_recover_cosets(self, nbits, lbits, index, ys_mont, length, evals=False):
        """A polynomial of `length` coefficients back from a subset of its cosets (kgs_kzg_recover_cosets): see
        the module-level kzg_recover_cosets."""
        return _kzg_recover_cosets(self._h, nbits, lbits, index, ys_mont, length, evals)

    def kzg_recover_cosets_device(self, nbits, lbits, d_index, d_ys, count, length, d_coef, d_evals=None):
        """Device-resident twin (kgs_kzg_recover_cosets_device): device pointers (ints) to count x uint64 coset
        indices and count * 2^lbits x 32 B Montgomery values, both only read, to length x 32 writable bytes and,
        or None, to 2^nbits x 32 writable bytes. Returns the verdict as a bool."""
        return _check(lib().kgs_kzg_recover_cosets_device(self._h, nbits, lbits, d_index, d_ys, count, length, d_coef,
                                                          d_evals)) == 1

    def kzg_recover_cosets_many(self, nbits, lbits, poly_of, index, ys_mont, length, polys, evals=False, stride=None,
                                coefs_out=None):
        """Many polynomials back from their cells in one call (kgs_kzg_recover_cosets_many): see the module-level
        kzg_recover_cosets_many. stride (>= length, default length): polynomial b's coefficients go to element
        stride * b of the result; coefs_out: a bytearray of polys * stride * 32 B that receives them in place (the gaps
        between length and stride are not written) and is returned as bytes."""
        return _kzg_recover_cosets_many(self._h, nbits, lbits, poly_of, index, ys_mont, length, polys, evals, stride,
                                        coefs_out)

    def kzg_recover_cosets_many_device(self, nbits, lbits, polys, d_poly_of, d_index, d_ys, count, length, stride, d_coef,
                                       d_evals=None, status=True):
        """Device-resident twin (kgs_kzg_recover_cosets_many_device): device pointers (ints) to count x uint32
        polynomial numbers, count x uint64 coset indices and count * 2^lbits x 32 B Montgomery values, all only read,
        to polys * stride x 32 writable bytes (polynomial b at 32 * stride * b; only its first `length` elements are
        written) and, or None, to polys * 2^nbits x 32 writable bytes. Returns (all recovered, list of statuses), or
        with status=False (status_out NULL) the bool alone."""
        st = ctypes.create_string_buffer(max(polys, 1)) if status else None
        rc = _check(lib().kgs_kzg_recover_cosets_many_device(self._h, nbits, lbits, polys, d_poly_of, d_index, d_ys, count,
                                                             length, stride, d_coef, d_evals, st))
        return (rc == 1, list(st.raw[:polys])) if status else rc == 1

    def last_exchange(self):
        """Exchanges of the last proof (kgs_last_exchange): all-to-all count / summed span ms / bytes
        sent, host all-gather count / wall ms / bytes sent; zeros after a single-GPU proof."""
        arr = (ctypes.c_double * 6)()
        lib().kgs_last_exchange(self._h, arr, 6)
        return {"alltoall_n": int(arr[0]), "alltoall_ms": arr[1], "alltoall_bytes": int(arr[2]),
                "allgather_n": int(arr[3]), "allgather_ms": arr[4], "allgather_bytes": int(arr[5])}

    def idle(self):
        """True when none of the context's streams has work outstanding (kgs_ctx_idle)."""
        rc = lib().kgs_ctx_idle(self._h)
        _check(rc)
        return rc == 1

    def last_timing(self):
        arr = (ctypes.c_double * 9)()
        n = lib().kgs_last_timing(self._h, arr, 9)
        return list(arr[:max(n, 0)])

    # ---- full prover ----
    def prove(self, kind, nbits, evals_f, evals_t, sel_f=None, sel_t=None, mont_out=True):
        """Host-buffer prover; returns (commitment list, evaluation list, mont_f, mont_t). Inputs
        are read in place; the Montgomery forms come back as bytearrays (no extra copies).
        mont_out: True (new bytearrays), False (no write-back), or a pair of lists (mont_f, mont_t)
        of writable caller buffers of 32 * 2^nbits bytes each that receive the Montgomery forms (a
        caller that recycles its output buffers, as the JS module's pool does)."""
        k = len(evals_f)
        n = 1 << nbits
        if any(len(x) != 32 * n for x in list(evals_f) + list(evals_t)):
            raise ValueError("evaluation buffers must hold 2^nbits 32-byte elements")
        given = None
        if isinstance(mont_out, (tuple, list)):
            given = (list(mont_out[0]), list(mont_out[1]))
            if len(given[0]) != k or len(given[1]) != k or any(len(x) != 32 * n for x in given[0] + given[1]):
                raise ValueError("write-back buffers must be two lists of npols buffers of 2^nbits 32-byte elements")
        keep = []
        PF = (ctypes.c_void_p * k)()
        PT = (ctypes.c_void_p * k)()
        MF = (ctypes.c_void_p * k)()
        MT = (ctypes.c_void_p * k)()
        mf, mt = [], []
        for i in range(k):
            (pf, kf), (pt, kt) = _ptr(evals_f[i]), _ptr(evals_t[i])
            keep += [kf, kt]
            PF[i], PT[i] = pf, pt
            if mont_out:
                ma, mb = (given[0][i], given[1][i]) if given else (_uninit_bytearray(32 * n), _uninit_bytearray(32 * n))
                (pa, ka), (pb, kb) = _ptr(ma), _ptr(mb)
                keep += [ka, kb]
                mf.append(ma)
                mt.append(mb)
                MF[i], MT[i] = pa, pb
        selected = sel_f is not None
        nc, ne = ctypes.c_int(), ctypes.c_int()
        lib().kgs_proof_shape(kind, k, 1 if selected else 0, ctypes.byref(nc), ctypes.byref(ne))
        com = ctypes.create_string_buffer(64 * nc.value)
        ev = ctypes.create_string_buffer(32 * ne.value)
        sf = st = None
        if selected:
            (sf, ksf), (st, kst) = _ptr(sel_f), _ptr(sel_t)
            keep += [ksf, kst]
        _check(lib().kgs_prove(self._h, kind, nbits, k, PF, PT, sf, st, MF if mont_out else None,
                               MT if mont_out else None, com, ev))
        coms = [com.raw[64 * i:64 * i + 64] for i in range(nc.value)]
        evs = [ev.raw[32 * i:32 * i + 32] for i in range(ne.value)]
        return coms, evs, mf, mt

    def prove_device(self, kind, nbits, d_f, d_t, d_sf=None, d_st=None):
        """Device-resident prover (d_* are device pointers as ints). Returns (commitments, evaluations)."""
        k = len(d_f)
        PF = (ctypes.c_void_p * k)(*d_f)
        PT = (ctypes.c_void_p * k)(*d_t)
        selected = d_sf is not None
        nc, ne = ctypes.c_int(), ctypes.c_int()
        lib().kgs_proof_shape(kind, k, 1 if selected else 0, ctypes.byref(nc), ctypes.byref(ne))
        com = ctypes.create_string_buffer(64 * nc.value)
        ev = ctypes.create_string_buffer(32 * ne.value)
        _check(lib().kgs_prove_device(self._h, kind, nbits, k, PF, PT, d_sf, d_st, com, ev))
        return ([com.raw[64 * i:64 * i + 64] for i in range(nc.value)],
                [ev.raw[32 * i:32 * i + 32] for i in range(ne.value)])


    def _prove_multi(self, fn, nbits, args, ptr):
        m = len(args)
        recs = (Arg * max(m, 1))()
        shapes, keep = [], []
        for j, (kind, fs, ts, sf, st) in enumerate(args):
            k = len(fs)
            PF = (ctypes.c_void_p * max(k, 1))()
            PT = (ctypes.c_void_p * max(k, 1))()
            for i in range(min(k, len(ts))):
                (PF[i], kf), (PT[i], kt) = ptr(fs[i]), ptr(ts[i])
                keep += [kf, kt]
            psf = pst = None
            if sf is not None:
                (psf, k1), (pst, k2) = ptr(sf), ptr(st)
                keep += [k1, k2]
            keep += [PF, PT]
            recs[j] = Arg(kind, k, PF, PT, psf, pst)
            shapes.append((kind, k, sf is not None))
        try:
            nc, ne = multi_proof_shape(shapes)
        except KgsError:
            nc = ne = 1  # the prover rejects these shapes below, with its own message, before it writes
        com = ctypes.create_string_buffer(64 * nc)
        ev = ctypes.create_string_buffer(32 * ne)
        _check(fn(self._h, nbits, recs, m, com, ev))
        return [com.raw[64 * i:64 * i + 64] for i in range(nc)], [ev.raw[32 * i:32 * i + 32] for i in range(ne)]

    def prove_multi(self, nbits, args):
        """Multi-argument prover on host buffers (kgs_prove_multi): args is a list of
        (kind, evals_f, evals_t, sel_f, sel_t) with evals_f / evals_t lists of standard-form buffers of
        2^nbits 32-byte elements and sel_f / sel_t Montgomery buffers or both None. Inputs are read in
        place and left as they are. Returns (commitment list, evaluation list) in the order of kgs.h."""
        n = 1 << nbits
        for a in args:
            bufs = list(a[1]) + list(a[2]) + [x for x in a[3:5] if x is not None]
            if any(len(x) != 32 * n for x in bufs):
                raise ValueError("evaluation buffers must hold 2^nbits 32-byte elements")
            if (a[3] is None) != (a[4] is None):
                raise ValueError("selectors must be both given or both None")
        return self._prove_multi(lib().kgs_prove_multi, nbits, args, _ptr)

    def prove_multi_device(self, nbits, args):
        """Device-resident twin (kgs_prove_multi_device): the same tuples with device pointers (ints)."""
        return self._prove_multi(lib().kgs_prove_multi_device, nbits, args, lambda p: (p, None))


def multi_proof_shape(shapes):
    """(commitments, evaluations) of a multi-argument proof (kgs_multi_proof_shape); shapes is a list of
    (kind, npols, selected)."""
    arr = (ArgShape * max(len(shapes), 1))(*[ArgShape(k, p, 1 if s else 0) for k, p, s in shapes])
    nc, ne = ctypes.c_int(), ctypes.c_int()
    rc = lib().kgs_multi_proof_shape(arr, len(shapes), ctypes.byref(nc), ctypes.byref(ne))
    if rc < 0:
        raise KgsError(rc, "bad multi-argument shapes")
    return nc.value, ne.value


def proof_names_multi(shapes):
    """Commitment / evaluation key order of a multi-argument proof (kgs.h): shapes is a list of
    (kind, npols, selected). One argument: proof_names's. More: every argument's names prefixed with
    "A<j>." ("A0.F", "A1.T2", "A1.selF", "A0.S", "A1.Z", "A0.fxi", "A1.zxiw"); Q, Wxi, Wxiw keep theirs."""
    if len(shapes) == 1:
        return proof_names(*shapes[0])
    com, com_s, ev, ev_s = [], [], [], []
    for j, (kind, npols, selected) in enumerate(shapes):
        cn, en = proof_names(kind, npols, selected)
        com += [f"A{j}.{x}" for x in cn[:-4]]
        com_s.append(f"A{j}.{cn[-4]}")
        ev += [f"A{j}.{x}" for x in en[:-1]]
        ev_s.append(f"A{j}.{en[-1]}")
    return com + com_s + ["Q", "Wxi", "Wxiw"], ev + ev_s


def dist_exchange_model(kind, nbits, npols, selected, world):
    """All-to-alls of one distributed proof (csrc/prover_dist.cpp) and the bytes that
    leave each rank in them: round 1 one per F_i / T_i (+ selectors) at n; round 2 S BLOCK -> E and its
    inverse at n, the coset forward transforms of S, F, T (+ selectors) at the coset size cs; round 3
    the quotient's inverse at cs; round 5 the two numerators CYCLIC -> BLOCK and the two openings
    BLOCK -> CYCLIC (one at cs, one at n each). An all-to-all of a length-L vector sends L / W^2
    elements to each of the W - 1 other ranks."""
    n = 1 << nbits
    gs = kind != GRANDPRODUCT
    cs = n if (not gs and not selected) else 2 * n
    sel = 2 if selected else 0
    lens = [n] * (2 * npols + sel) + [n, n] + [cs] * (3 + sel) + [cs] + [cs, n, cs, n]
    W = world
    return {"alltoall_n": len(lens), "alltoall_bytes": sum(32 * (L // (W * W)) * (W - 1) for L in lens)}


def proof_names(kind, npols, selected):
    """Commitment / evaluation key order of the C-ABI outputs (kgs.h) in the reference's names."""
    vec = npols > 1
    gs = kind != GRANDPRODUCT
    com = []
    for i in range(npols):
        com += [f"F{i}" if vec else "F", f"T{i}" if vec else "T"]
    if selected:
        com += ["selF", "selT"]
    com += ["S" if gs else "Z", "Q", "Wxi", "Wxiw"]
    ev = []
    for i in range(npols):
        ev.append(f"f{i}xi" if vec else "fxi")
        if gs:
            ev.append(f"t{i}xi" if vec else "txi")
    if selected:
        ev += ["selFxi", "selTxi"]
    ev.append("sxiw" if gs else "zxiw")
    return com, ev


_CTX = {}


def _context(device=0):
    if device not in _CTX:
        _CTX[device] = Context(device)
    return _CTX[device]


def _prover_inputs(kind, power, evalsFs, evalsTs, evalsSelF, evalsSelT):
    """src/grandsum/mset_eq_kzg_prover.js:22-81 — the input checks with the reference's messages.
    -> (evalsFs, evalsTs, evalsSelF, evalsSelT, is_selected, nbits)"""
    if not isinstance(evalsFs, (list, tuple)):
        evalsFs = [evalsFs]
    if not isinstance(evalsTs, (list, tuple)):
        evalsTs = [evalsTs]
    if len(evalsFs) != len(evalsTs):
        raise ValueError("The lengths of the two vector multisets must be the same.")
    npols = len(evalsFs)
    if npols == 0:
        raise ValueError("The number of multisets must be greater than 0.")
    for i in range(npols):
        if evalsFs[i].length() != evalsTs[i].length():
            raise ValueError(f"The {i}-th multiset buffers must have the same length.")
        elif evalsFs[i].length() != evalsFs[0].length():
            raise ValueError("The multiset buffers must all have the same length.")
    n0 = evalsFs[0].length()
    if kind == LOOKUP and evalsSelT is None:
        raise ValueError("A lookup needs the multiplicities of the table.")
    if evalsSelF is None:
        evalsSelF = Evaluations.getOneEvals(n0)
    if evalsSelT is None:
        evalsSelT = Evaluations.getOneEvals(n0)
    if evalsSelF.length() != evalsSelT.length():
        raise ValueError("The selection buffers must have the same length.")
    elif evalsSelF.length() != n0:
        raise ValueError("The selection buffers must have the same length as the multiset buffers.")
    # a lookup keeps its selectors even when all one (its proof always carries selF / selT)
    is_selected = kind == LOOKUP or not (evalsSelF.isAllOnes() and evalsSelT.isAllOnes())
    if is_selected and evalsSelF.isAllZeros() and evalsSelT.isAllZeros():  # prover.js:66-68
        log.warning("The selection buffers are all zeros. The argument is trivially satisfied.")
    nbits = (n0 - 1).bit_length() if n0 > 0 else 0
    if n0 != (1 << nbits):
        raise ValueError("Polynomial length must be a power of two.")
    if power < nbits:
        raise ValueError("The Powers of Tau file is not sufficiently large to commit the polynomials.")
    return evalsFs, evalsTs, evalsSelF, evalsSelT, is_selected, nbits


def _prover(kind, pTauFilename, evalsFs, evalsTs, evalsSelF=None, evalsSelT=None, device=0):
    """src/grandsum/mset_eq_kzg_prover.js:12-142 — input checks with the reference's messages, then
    the HIP prover. Overwrites evalsFs[i].eval / evalsTs[i].eval with Montgomery form (:147-148)."""
    log.info("> MULTISET EQUALITY KZG %s PROVER STARTED", _TITLE[kind])
    power = ptau_power(pTauFilename)  # the header is read first (prover.js:15-16)
    evalsFs, evalsTs, evalsSelF, evalsSelT, is_selected, nbits = _prover_inputs(kind, power, evalsFs, evalsTs,
                                                                                evalsSelF, evalsSelT)
    npols = len(evalsFs)
    if log.isEnabledFor(logging.INFO):  # prover.js:87-93
        for line in ("-------------------------------------", f"  MULTISET EQUALITY KZG {_TITLE[kind]} PROVER SETTINGS",
                     "  Curve:       bn128", f"  Domain size: {1 << nbits}", f"  Number of polynomials: {npols}",
                     f"  Selectors: {'Yes' if is_selected else 'No'}", "-------------------------------------"):
            log.info(line)
    ctx = _context(device)
    # the drop-in functions follow the environment on every call (contexts are cached per device)
    ctx.set_reference_quirks(os.environ.get("KGS_REFERENCE_QUIRKS", "1") != "0")
    # only the 2^(nbits+1) points this proof commits with (prover.js:83-85); grow-only device cache
    ctx.load_ptau(pTauFilename, nbits)
    coms, evs, mf, mt = ctx.prove(kind, nbits, [e.eval for e in evalsFs], [e.eval for e in evalsTs],
                                  evalsSelF.eval if is_selected else None,
                                  evalsSelT.eval if is_selected else None)
    for i in range(npols):
        evalsFs[i].eval = mf[i]
        evalsTs[i].eval = mt[i]
    cn, en = proof_names(kind, npols, is_selected)
    proof = {"commitments": dict(zip(cn, coms)), "evaluations": dict(zip(en, evs))}
    if log.isEnabledFor(logging.INFO):
        log_rounds(kind, proof, nbits, npols, is_selected)
    return proof


# ---------------------------------------------------------------- the reference's log lines
# logger.js (logplease at INFO) as used by src/grandsum/mset_eq_kzg_prover.js:13-140,164-412 and the
# grand-product twin: the same messages on the standard `logging` logger "kgs" (silent until the
# caller enables INFO on it). The proof is computed in one library call, so the round lines follow
# it, with the challenges replayed from the proof's transcript (src/Keccak256Transcript.js:7-53).
import logging  # noqa: E402

log = logging.getLogger("kgs")
_FQ = 21888242871839275222246405745257275088696311157297823662689037894645226208583
_FR = 21888242871839275222246405745257275088548364400416034343698204186575808495617
_TITLE = {GRANDSUM: "GRAND-SUM", GRANDPRODUCT: "GRAND-PRODUCT", LOOKUP: "GRAND-SUM (LOOKUP)"}


def _fr_int(b):  # 32 B LE Montgomery Fr -> integer
    return int.from_bytes(bytes(b), "little") * pow(1 << 256, _FR - 2, _FR) % _FR


def _g1_xy(b):  # 64 B affine LEM -> (x, y) standard, None for the zero point
    rinv = pow(1 << 256, _FQ - 2, _FQ)
    x = int.from_bytes(bytes(b[:32]), "little") * rinv % _FQ
    y = int.from_bytes(bytes(b[32:64]), "little") * rinv % _FQ
    return None if x == 0 and y == 0 else (x, y)


def _g1_str(b):  # [ffjs] G1.toString of an affine point
    a = _g1_xy(b)
    return "[ 0, 1, 0 ]" if a is None else f"[ {a[0]}, {a[1]}, 1 ]"


class _Transcript:
    """G1.toRprUncompressed (64 B big-endian x||y, the zero point 0x40 then zeros) / Fr.toRprBE (32 B);
    a challenge is keccak256 of everything added so far, big-endian, mod r."""

    def __init__(self):
        self.buf = bytearray()

    def add_commitment(self, b):
        a = _g1_xy(b)
        self.buf += (b"\x40" + bytes(63)) if a is None else a[0].to_bytes(32, "big") + a[1].to_bytes(32, "big")

    def add_scalar(self, v):
        self.buf += (v % _FR).to_bytes(32, "big")

    def challenge(self):
        return int.from_bytes(keccak256(bytes(self.buf)), "big") % _FR


def log_rounds(kind, proof, nbits, npols, selected, logger=None):
    """Write the reference's round log of `proof` (prover.js:111-140 with each round's lines) and
    return its challenges {beta, gamma, alpha, xi, v} (beta None for k = 1)."""
    lg = logger or log
    gs = kind != GRANDPRODUCT
    vec = npols > 1
    C, E = proof["commitments"], proof["evaluations"]
    tr = _Transcript()
    msg = "> ROUND ${round}. Generate the witness polynomials"  # printed literally by the reference
    msg += f" fᵢ,tᵢ ∈ 𝔽[X], for i ∈ [{npols}]" if vec else " f,t ∈ 𝔽[X]"
    if selected:
        msg += ", and the selector polynomials fsel,tsel ∈ 𝔽[X]"
    lg.info(msg)
    for i in range(npols):
        nf, nt = (f"F{i}", f"T{i}") if vec else ("F", "T")
        lg.info("··· [%s]₁ = %s", f"f{i + 1}(x)" if vec else "f(x)", _g1_str(C[nf]))
        lg.info("··· [%s]₁ = %s", f"t{i + 1}(x)" if vec else "t(x)", _g1_str(C[nt]))
        tr.add_commitment(C[nf])
        tr.add_commitment(C[nt])
    if selected:
        lg.info("··· [fsel(x)]₁ = %s", _g1_str(C["selF"]))
        lg.info("··· [tsel(x)]₁ = %s", _g1_str(C["selT"]))
        tr.add_commitment(C["selF"])
        tr.add_commitment(C["selT"])
    sz = "S" if gs else "Z"
    lg.info("> ROUND 2. Compute the grand-%s polynomial %s ∈ 𝔽[X]", "sum" if gs else "product", sz)
    beta = None
    if vec:
        beta = tr.challenge()
        lg.info("···      𝛃  = %d", beta)
        tr.add_scalar(beta)
    gamma = tr.challenge()
    lg.info("···      𝜸  = %d", gamma)
    lg.info("··· [%s(x)]₁ = %s", sz, _g1_str(C[sz]))
    lg.info("> ROUND 3. Compute the quotient polynomial Q ∈ 𝔽[X]")
    tr.add_scalar(gamma)
    tr.add_commitment(C[sz])
    alpha = tr.challenge()
    lg.info("···      𝜶  = %d", alpha)
    lg.info("··· [Q(x)]₁ = %s", _g1_str(C["Q"]))
    lg.info("> ROUND 4. Compute the evaluations of the polynomials")
    tr.add_scalar(alpha)
    tr.add_commitment(C["Q"])
    xi = tr.challenge()
    lg.info("···      𝔷  = %d", xi)
    evs = []
    for i in range(npols):
        fx = _fr_int(E[f"f{i}xi" if vec else "fxi"])
        lg.info("···   %s  = %d", f"f{i + 1}(𝔷)" if vec else "f(𝔷)", fx)
        evs.append(fx)
        if gs:
            tx = _fr_int(E[f"t{i}xi" if vec else "txi"])
            lg.info("···   %s  = %d", f"t{i + 1}(𝔷)" if vec else "t(𝔷)", tx)
            evs.append(tx)
    if selected:
        evs += [_fr_int(E["selFxi"]), _fr_int(E["selTxi"])]
        lg.info("···   fsel(𝔷)  = %d", evs[-2])
        lg.info("···   tsel(𝔷)  = %d", evs[-1])
    zw = _fr_int(E["sxiw" if gs else "zxiw"])
    lg.info("··· %s(𝔷·𝛚)  = %d", sz, zw)
    lg.info("> ROUND 5. Compute the opening proof polynomials W𝔷, W𝔷𝛚 ∈ 𝔽[X]")
    tr.add_scalar(xi)
    for v in evs + [zw]:
        tr.add_scalar(v)
    v = tr.challenge()
    lg.info("···      v  =  %d", v)
    n = 1 << nbits
    zh = (pow(xi, n, _FR) - 1) % _FR  # polynomial_utils.js:1-19
    l1 = zh * pow(n * (xi - 1) % _FR, _FR - 2, _FR) % _FR
    lg.info("···  ZH(𝔷)  = %d", zh)
    lg.info("···  L₁(𝔷)  = %d", l1)
    lg.info("··· [W𝔷(x)]₁   = %s", _g1_str(C["Wxi"]))
    lg.info("··· [W𝔷·𝛚(x)]₁ = %s", _g1_str(C["Wxiw"]))
    lg.info("")
    lg.info("> MULTISET EQUALITY KZG %s PROVER FINISHED", _TITLE[kind])
    return {"beta": beta, "gamma": gamma, "alpha": alpha, "xi": xi, "v": v}


def grandsum_prover(pTauFilename, evalsFs, evalsTs, evalsSelF=None, evalsSelT=None, device=0):
    """mset_eq_kzg_grandsum_prover (src/grandsum/mset_eq_kzg_prover.js:12)."""
    try:
        return _prover(GRANDSUM, pTauFilename, evalsFs, evalsTs, evalsSelF, evalsSelT, device)
    except KgsError as e:
        raise _semantic(e) from e


def grandproduct_prover(pTauFilename, evalsFs, evalsTs, evalsSelF=None, evalsSelT=None, device=0):
    """mset_eq_kzg_grandproduct_prover (src/grandproduct/mset_eq_kzg_prover.js:12)."""
    try:
        return _prover(GRANDPRODUCT, pTauFilename, evalsFs, evalsTs, evalsSelF, evalsSelT, device)
    except KgsError as e:
        raise _semantic(e) from e


def _verifier(kind, pTauFilename, proof, nBits):
    """src/{grandsum,grandproduct}/mset_eq_kzg_verifier.js:9 — the proof's shape is read from its
    keys as the reference does (nPols from /^F[0-9]/, selectors from /^selF/); the check runs in
    libkgs (kgs_verify_ptau: transcript replay + optimal-ate pairing, host only)."""
    shape = _proof_buffers(kind, proof)
    if shape is None:
        return False
    npols, selected, com, ev = shape
    rc = _check(lib().kgs_verify_ptau(kind, os.fsencode(pTauFilename), nBits, npols, 1 if selected else 0,
                                      _buf(com), _buf(ev)))
    return rc == 1


def _proof_buffers(kind, proof):
    """(npols, selected, commitments, evaluations) of a proof dict in the C-ABI order, its shape read
    from its keys; None for a proof that is invalid before the library sees it (a missing key, a value
    of the wrong length, a lookup without selectors)."""
    import re
    keys = list(proof["commitments"].keys())
    nfi = len([k for k in keys if re.match(r"^F\d", k)])
    npols = nfi if nfi > 0 else 1
    selected = len([k for k in keys if re.match(r"^selF", k)]) == 1
    if kind == LOOKUP and not selected:
        return None
    cn, en = proof_names(kind, npols, selected)
    try:
        com = b"".join(bytes(proof["commitments"][n]) for n in cn)
        ev = b"".join(bytes(proof["evaluations"][n]) for n in en)
    except KeyError:
        return None
    if len(com) != 64 * len(cn) or len(ev) != 32 * len(en):
        return None
    return npols, selected, com, ev


def _verify_batch(handle, items, tau_g2, ptau, locate, diag):
    if (tau_g2 is None) == (ptau is None):
        raise ValueError("give exactly one of tau_g2 and ptau")
    items = list(items)
    sent = []  # positions of the items that reach the library
    keep = []
    for pos, (kind, proof, nBits) in enumerate(items):
        shape = _proof_buffers(kind, proof)
        if shape is not None:
            sent.append(pos)
            keep.append((kind, nBits) + shape)
    n = len(sent)
    refs = (ProofRef * max(n, 1))()
    bufs = []
    for j, (kind, nBits, npols, selected, com, ev) in enumerate(keep):
        cb, eb = _buf(com), _buf(ev)
        bufs += [cb, eb]
        refs[j] = ProofRef(kind, nBits, npols, 1 if selected else 0, ctypes.cast(cb, ctypes.c_void_p),
                           ctypes.cast(eb, ctypes.c_void_p))
    valid = ctypes.create_string_buffer(max(n, 1)) if locate else None
    d = BatchDiag()
    w = f = None
    if diag is not None:
        w, f = ctypes.create_string_buffer(32 * max(n, 1)), ctypes.create_string_buffer(128 * max(n, 1))
        d.weights_out, d.folded_out = ctypes.cast(w, ctypes.c_void_p), ctypes.cast(f, ctypes.c_void_p)
    if ptau is not None:
        rc = lib().kgs_verify_batch_ptau(handle, os.fsencode(ptau), refs, n, valid, ctypes.byref(d))
    else:
        rc = lib().kgs_verify_batch(handle, refs, n, _buf(tau_g2), valid, ctypes.byref(d))
    _check(rc)
    if diag is not None:
        diag.update(indices=sent, weights=w.raw[:32 * n], folded=f.raw[:128 * n], pairing_checks=d.pairing_checks,
                    terms=d.terms, on_gpu=d.on_gpu, fold_ms=d.fold_ms, pairing_ms=d.pairing_ms)
    if not locate:
        return rc == 1 and n == len(items)
    out = [False] * len(items)
    for j, pos in enumerate(sent):
        out[pos] = valid.raw[j] == 1
    return out


def verify_batch(pTauFilename, items, device=0, locate=True, diag=None):
    """Verify many proofs against one ptau's [tau]_2 with ONE pairing check (include/kgs.h
    kgs_verify_batch). items: a sequence of (kind, proof, nBits) with kind GRANDSUM / GRANDPRODUCT /
    LOOKUP and proof the dict the provers return; each proof's shape is read from its keys as the
    single-proof verifiers do. Returns a list of bool, item for item what grandsum_verifier /
    grandproduct_verifier / lookup_verifier return; an item with a missing key, a value of the wrong
    length or a lookup without selectors is False without reaching the library.
    device: the GPU whose context folds the proofs' commitments; None folds on the host (no GPU).
    locate=False stops after the aggregate check and returns one bool (all valid).
    diag: a dict that receives indices (positions of the items sent to the library; the entries below
    are in that order), weights (32 B each), folded (128 B each: rho A || rho B), pairing_checks, terms,
    on_gpu, fold_ms, pairing_ms."""
    handle = None if device is None else _context(device).handle
    return _verify_batch(handle, items, None, pTauFilename, locate, diag)


def _g1_lincomb(handle, points_lem, scalars_std, seg_off):
    seg_off = list(seg_off)
    if not seg_off:
        raise ValueError("seg_off holds the number of segments + 1 offsets")
    nseg = len(seg_off) - 1
    nterms = seg_off[-1]
    if len(points_lem) != 64 * nterms or len(scalars_std) != 32 * nterms:
        raise ValueError("points_lem / scalars_std must hold seg_off[-1] points of 64 B / scalars of 32 B")
    off = (ctypes.c_uint64 * (nseg + 1))(*seg_off)
    out = ctypes.create_string_buffer(max(64 * nseg, 1))
    _check(lib().kgs_g1_lincomb(handle, _buf(points_lem), _buf(scalars_std), off, nseg, out))
    return out.raw[:64 * nseg]


def g1_lincomb(points_lem, scalars_std, seg_off, device=0):
    """out[s] = sum over t in [seg_off[s], seg_off[s + 1]) of scalars[t] * points[t] (kgs_g1_lincomb):
    points 64 B affine LEM (the zero point allowed), scalars 32 B little-endian standard form (any
    256-bit integer), seg_off the nseg + 1 term offsets. Returns nseg x 64 B affine LEM (zeros for the
    identity). device=None computes on the host."""
    handle = None if device is None else _context(device).handle
    return _g1_lincomb(handle, points_lem, scalars_std, seg_off)


def _msm_points(handle, points_lem, scalars_std, window_c):
    if len(points_lem) % 64 or len(scalars_std) % 32 or len(points_lem) // 64 != len(scalars_std) // 32:
        raise ValueError("points_lem / scalars_std must hold the same number of 64 B points / 32 B scalars")
    n = len(points_lem) // 64
    out = ctypes.create_string_buffer(64)
    (pp, kp), (ps, ks) = _ptr(points_lem), _ptr(scalars_std)  # read in place
    _check(lib().kgs_msm_points(handle, pp if n else None, ps if n else None, n, window_c, out))
    del kp, ks
    return out.raw


def msm_points(points_lem, scalars_std, device=0, window_c=0):
    """sum_i scalars[i] * points[i] over arbitrary bases (kgs_msm_points), without window tables: points
    64 B affine LEM (the zero point allowed, points are not validated), scalars 32 B little-endian
    standard form (any 256-bit integer, taken mod r). Returns 64 B affine LEM (zeros for the identity).
    window_c: 0 lets the library choose, 7 .. 16 sets the Pippenger window. device=None computes on the
    host."""
    handle = None if device is None else _context(device).handle
    return _msm_points(handle, points_lem, scalars_std, window_c)


def _g1_ntt(handle, points_lem, inverse):
    m = len(points_lem) // 64
    if len(points_lem) % 64 or m == 0 or m & (m - 1):
        raise ValueError("points_lem must hold a power of two of 64 B points")
    out = ctypes.create_string_buffer(64 * m)
    pp, kp = _ptr(points_lem)  # read in place
    _check(lib().kgs_g1_ntt(handle, pp, out, m.bit_length() - 1, 1 if inverse else 0))
    del kp
    return out.raw


def g1_ntt(points_lem, inverse=False, device=0):
    """[ffjs] G1.fft / G1.ifft (kgs_g1_ntt): the number-theoretic transform over G1 of 2^logm affine LEM
    points of 64 B (the zero point allowed, points are not validated), natural order in and out, with the
    root Fr.w[logm] of the Fr transform: out_j = sum_i w^(ij) P_i, inverse out_j = (1/m) sum_i w^(-ij) P_i.
    Returns 2^logm x 64 B canonical affine LEM. device=None computes on the host."""
    handle = None if device is None else _context(device).handle
    return _g1_ntt(handle, points_lem, inverse)


def commit_evals(pTauFilename, evals, device=0):
    """The commitment to the polynomial with the evaluations `evals` (standard-form Evaluations, or a
    bytes-like of 2^nbits 32-byte elements) on the domain of their length, over the SRS of pTauFilename
    (kgs_commit_evals): the Lagrange bases are built on first use and cached on the device. Returns 64 B
    affine LEM."""
    data = evals.eval if isinstance(evals, Evaluations) else evals
    m = len(data) // 32
    if len(data) % 32 or m == 0 or m & (m - 1):
        raise ValueError("evals must hold a power of two of 32-byte elements")
    nbits = m.bit_length() - 1
    ctx = _context(device)
    ctx.load_ptau(pTauFilename, nbits)
    return ctx.commit_evals(data, nbits)


def _g1_mul_each(handle, points_lem, scalars_std):
    if len(points_lem) % 64 or len(scalars_std) % 32 or len(points_lem) // 64 != len(scalars_std) // 32:
        raise ValueError("points_lem / scalars_std must hold the same number of 64 B points / 32 B scalars")
    n = len(points_lem) // 64
    out = ctypes.create_string_buffer(max(64 * n, 1))
    (pp, kp), (ps, ks) = _ptr(points_lem), _ptr(scalars_std)  # read in place
    _check(lib().kgs_g1_mul_each(handle, pp if n else None, ps if n else None, n, out))
    del kp, ks
    return out.raw[:64 * n]


def g1_mul_each(points_lem, scalars_std, device=0):
    """out[i] = scalars[i] * points[i] (kgs_g1_mul_each): points 64 B affine LEM (the zero point allowed,
    points are not validated), scalars 32 B little-endian standard form (any 256-bit integer, taken mod
    r). Returns n x 64 B canonical affine LEM (zeros for the identity). device=None computes on the host."""
    handle = None if device is None else _context(device).handle
    return _g1_mul_each(handle, points_lem, scalars_std)


def kzg_open_all(pTauFilename, coefs, device=0):
    """All openings of the polynomial with the Montgomery coefficients `coefs` (a bytes-like of 32-byte
    elements) on the smallest domain 2^nbits that holds them, over the SRS of pTauFilename
    (kgs_kzg_open_all): returns (proofs, evals), 2^nbits x 64 B affine LEM and 2^nbits x 32 B Montgomery,
    entry i for the point Fr.w[nbits]^i."""
    if len(coefs) % 32:
        raise ValueError("coefs must hold 32-byte elements")
    nbits = max(len(coefs) // 32 - 1, 0).bit_length()
    ctx = _context(device)
    ctx.load_ptau(pTauFilename, nbits)
    return ctx.kzg_open_all(coefs, nbits, evals=True)


def kzg_verify(tau_g2, commit, z_mont, y_mont, proof):
    """The check of one KZG opening on the host (kgs_kzg_verify): e(proof, [tau]_2) ==
    e(commit - y G + z proof, [1]_2). tau_g2: 128 B LEM, or the name of a ptau file to read it from;
    commit / proof 64 B affine LEM, z_mont / y_mont 32 B Montgomery. Returns a bool; a commitment or proof
    that is no point of the curve is False."""
    if len(commit) != 64 or len(proof) != 64 or len(z_mont) != 32 or len(y_mont) != 32:
        raise ValueError("commit / proof hold 64 bytes, z_mont / y_mont 32")
    if isinstance(tau_g2, (str, os.PathLike)) or len(tau_g2) != 128:
        t2 = ctypes.create_string_buffer(128)
        _check(lib().kgs_ptau_read_tau_g2(os.fsencode(tau_g2), t2))
        tau_g2 = t2.raw
    return _check(lib().kgs_kzg_verify(_buf(commit), _buf(z_mont), _buf(y_mont), _buf(proof), _buf(tau_g2))) == 1


def _g1_mul_sum(handle, points_lem, scalars_std, rows):
    n = len(points_lem) // 64
    if len(points_lem) % 64 or len(scalars_std) % 32 or n != len(scalars_std) // 32 or rows < 1 or n % rows:
        raise ValueError("points_lem / scalars_std must hold the same rows * cols 64 B points / 32 B scalars")
    cols = n // rows
    out = ctypes.create_string_buffer(max(64 * cols, 1))
    (pp, kp), (ps, ks) = _ptr(points_lem), _ptr(scalars_std)  # read in place
    _check(lib().kgs_g1_mul_sum(handle, pp if n else None, ps if n else None, rows, cols, out))
    del kp, ks
    return out.raw[:64 * cols]


def g1_mul_sum(points_lem, scalars_std, rows, device=0):
    """out[i] = sum_{r < rows} scalars[r cols + i] * points[r cols + i] (kgs_g1_mul_sum), cols = the number of
    terms / rows: points 64 B affine LEM (the zero point allowed, not validated), scalars 32 B little-endian
    standard form (any 256-bit integer, taken mod r). Returns cols x 64 B canonical affine LEM (zeros for the
    identity). device=None computes on the host."""
    handle = None if device is None else _context(device).handle
    return _g1_mul_sum(handle, points_lem, scalars_std, rows)


def kzg_open_cosets(pTauFilename, coefs, lbits, device=0):
    """Every coset opening of the polynomial with the Montgomery coefficients `coefs` on the smallest domain
    2^nbits that holds them and 2^lbits points, over the SRS of pTauFilename (kgs_kzg_open_cosets): returns
    (proofs, evals), 2^(nbits - lbits) x 64 B affine LEM, proof i for the values evals[i + 2^(nbits - lbits) j],
    and 2^nbits x 32 B Montgomery."""
    if len(coefs) % 32:
        raise ValueError("coefs must hold 32-byte elements")
    nbits = max(max(len(coefs) // 32 - 1, 0).bit_length(), lbits)
    ctx = _context(device)
    ctx.load_ptau(pTauFilename, nbits)
    return ctx.kzg_open_cosets(coefs, nbits, lbits, evals=True)


def kzg_open_cosets_many(pTauFilename, coefs, lbits, device=0):
    """Every coset opening of each polynomial of the list `coefs` (bytes-likes of Montgomery coefficients) on the
    smallest domain 2^nbits that holds the longest of them and 2^lbits points, over the SRS of pTauFilename, in one
    call (kgs_kzg_open_cosets_many): returns (list of proofs, list of evaluations), each entry what kzg_open_cosets
    returns for that polynomial on that domain."""
    coefs = [bytes(c) for c in coefs]
    if any(len(c) % 32 for c in coefs):
        raise ValueError("coefs must hold 32-byte elements")
    longest = max((len(c) // 32 for c in coefs), default=0)
    nbits = max(max(longest - 1, 0).bit_length(), lbits)
    ctx = _context(device)
    ctx.load_ptau(pTauFilename, nbits)
    return ctx.kzg_open_cosets_many(coefs, nbits, lbits, evals=True)


def ptau_read_tau_g2_pow(pTauFilename, k):
    """[tau^k]_2, point k of the ptau's section 3, as 128 B LEM (kgs_ptau_read_tau_g2_pow); a file that holds
    fewer points raises KgsError (KGS_E_IO)."""
    out = ctypes.create_string_buffer(128)
    _check(lib().kgs_ptau_read_tau_g2_pow(os.fsencode(pTauFilename), k, out))
    return out.raw


def kzg_verify_coset(tau_l_g2, srs_g1, commit, nbits, lbits, index, ys_mont, proof):
    """The check of one coset opening on the host (kgs_kzg_verify_coset): proof opens commit to the 2^lbits
    values ys_mont (32 B Montgomery each, ys[j] = p(w^(index + m j)), m = 2^(nbits - lbits)) on coset
    `index`. tau_l_g2: [tau^l]_2 as 128 B LEM, or the name of a ptau file to read it from; srs_g1: the first
    2^lbits points [tau^k]_1 as 64 B affine LEM (more are ignored). Returns a bool; a point off the curve or
    a value not below r is False."""
    l = 1 << lbits if 0 <= lbits <= 28 else 0
    if len(commit) != 64 or len(proof) != 64 or len(ys_mont) != 32 * l or len(srs_g1) < 64 * l:
        raise ValueError("commit / proof hold 64 bytes, ys_mont 2^lbits x 32, srs_g1 at least 2^lbits x 64")
    if isinstance(tau_l_g2, (str, os.PathLike)) or len(tau_l_g2) != 128:
        tau_l_g2 = ptau_read_tau_g2_pow(tau_l_g2, l)
    return _check(lib().kgs_kzg_verify_coset(_buf(commit), nbits, lbits, index, _buf(ys_mont), _buf(proof),
                                             _buf(srs_g1[:64 * l]), _buf(tau_l_g2))) == 1


def _commit_bytes(commits):
    if isinstance(commits, (bytes, bytearray, memoryview)):
        data = bytes(commits)
    else:
        commits = [bytes(c) for c in commits]
        if any(len(c) != 64 for c in commits):
            raise ValueError("a commitment holds 64 bytes")
        data = b"".join(commits)
    if len(data) % 64:
        raise ValueError("commits must hold 64-byte points")
    return data


def _coset_batch_call(fn, handle, tau_l_g2, srs_g1, nbits, lbits, commits, commit_of, index, ys, proofs, count, seed,
                      locate, diag):
    l = 1 << lbits if 0 <= lbits <= 28 else 0
    if isinstance(tau_l_g2, (str, os.PathLike)) or len(tau_l_g2) != 128:
        tau_l_g2 = ptau_read_tau_g2_pow(tau_l_g2, l)
    valid = ctypes.create_string_buffer(max(count, 1)) if locate else None
    d = CosetBatchDiag()
    rho = fo = it = None
    if diag is not None:
        rho, fo, it = ctypes.create_string_buffer(32), ctypes.create_string_buffer(128), \
            ctypes.create_string_buffer(32 * max(l, 1))
        d.rho_out, d.folded_out, d.interp_out = (ctypes.cast(x, ctypes.c_void_p) for x in (rho, fo, it))
    rc = _check(fn(handle, nbits, lbits, _buf(commits) if commits else None, len(commits) // 64, commit_of, index, ys,
                   proofs, count, _buf(srs_g1[:64 * l]), _buf(tau_l_g2), _buf(seed) if seed is not None else None,
                   valid, ctypes.byref(d)))
    if diag is not None:
        diag.update(rho=rho.raw, folded=fo.raw, interp=it.raw, pairing_checks=d.pairing_checks, on_gpu=d.on_gpu,
                    hash_ms=d.hash_ms, fold_ms=d.fold_ms, pairing_ms=d.pairing_ms)
    if not locate:
        return rc == 1
    return [valid.raw[k] == 1 for k in range(count)]


def _kzg_verify_cosets_batch(handle, tau_l_g2, srs_g1, nbits, lbits, commits, openings, locate, seed, diag):
    commits = _commit_bytes(commits)
    l = 1 << lbits if 0 <= lbits <= 28 else 0
    if len(srs_g1) < 64 * l:
        raise ValueError("srs_g1 must hold at least 2^lbits x 64 bytes")
    if seed is not None and len(seed) != 32:
        raise ValueError("seed holds 32 bytes")
    openings = list(openings)
    sent = []  # positions of the openings that reach the library
    for pos, (ci, idx, ys, proof) in enumerate(openings):
        if len(ys) == 32 * l and len(proof) == 64 and 0 <= ci < (1 << 32) and 0 <= idx < (1 << 64):
            sent.append(pos)
    n = len(sent)
    cof = (ctypes.c_uint32 * max(n, 1))(*[openings[p][0] for p in sent])
    index = (ctypes.c_uint64 * max(n, 1))(*[openings[p][1] for p in sent])
    ys = _buf(b"".join(bytes(openings[p][2]) for p in sent)) if n else None
    proofs = _buf(b"".join(bytes(openings[p][3]) for p in sent)) if n else None
    got = _coset_batch_call(lib().kgs_kzg_verify_cosets_batch, handle, tau_l_g2, srs_g1, nbits, lbits, commits,
                            ctypes.cast(cof, ctypes.c_void_p), ctypes.cast(index, ctypes.c_void_p), ys, proofs, n, seed,
                            locate, diag)
    if diag is not None:
        diag["indices"] = sent
    if not locate:
        return got and n == len(openings)
    out = [False] * len(openings)
    for j, pos in enumerate(sent):
        out[pos] = got[j]
    return out


def kzg_verify_cosets_batch(tau_l_g2_or_ptau, srs_g1, nbits, lbits, commits, openings, device=0, locate=True, seed=None,
                            diag=None):
    """Verify many coset openings against one SRS with ONE pairing check (include/kgs.h
    kgs_kzg_verify_cosets_batch). tau_l_g2_or_ptau: [tau^l]_2 as 128 B LEM, or the name of a ptau file to read it
    from; srs_g1: the first 2^lbits points [tau^k]_1 (64 B affine LEM each, more are ignored); commits: a list of
    64 B commitments (or their concatenation); openings: a sequence of (commit_index, coset_index, ys_mont, proof)
    with ys_mont the 2^lbits values of the coset (32 B Montgomery each) and proof 64 B affine LEM, as
    kzg_open_cosets gives them. Returns a list of bool, opening for opening what kzg_verify_coset returns; an
    opening with ys_mont or proof of the wrong length is False without reaching the library.
    device: the GPU whose context folds the batch; None computes on the host (no GPU). locate=False stops after
    the aggregate check and returns one bool (all valid). seed: None derives the weights from a hash of the whole
    batch; 32 bytes of the caller's replace that hash and must be unpredictable to whoever made the proofs.
    diag: a dict that receives indices (positions of the openings sent to the library), rho (32 B standard form),
    folded (A || B of the whole-batch check), interp (D, 2^lbits x 32 B Montgomery), pairing_checks, on_gpu,
    hash_ms, fold_ms, pairing_ms."""
    handle = None if device is None else _context(device).handle
    return _kzg_verify_cosets_batch(handle, tau_l_g2_or_ptau, srs_g1, nbits, lbits, commits, openings, locate, seed,
                                    diag)


def _coset_interp_fold(handle, nbits, lbits, index, ys_mont, weights_mont):
    index = list(index)
    count = len(index)
    l = 1 << lbits if 0 <= lbits <= 28 else 0
    if len(ys_mont) != 32 * l * count or len(weights_mont) != 32 * count:
        raise ValueError("ys_mont holds len(index) * 2^lbits and weights_mont len(index) 32-byte elements")
    idx = (ctypes.c_uint64 * max(count, 1))(*index)
    out = ctypes.create_string_buffer(32 * max(l, 1))
    _check(lib().kgs_coset_interp_fold(handle, nbits, lbits, ctypes.cast(idx, ctypes.c_void_p),
                                       _buf(ys_mont) if count else None, _buf(weights_mont) if count else None, count,
                                       out))
    return out.raw[:32 * l]


def coset_interp_fold(nbits, lbits, index, ys_mont, weights_mont, device=0):
    """D_j = sum_k weights[k] * w^(-index[k] j) * J_{k,j}, j < 2^lbits (kgs_coset_interp_fold): J_k is the inverse
    transform of size 2^lbits of row k of ys_mont (32 B Montgomery values, the rows contiguous), w = Fr.w[nbits];
    weights_mont holds one 32 B Montgomery weight per row. With one row of weight one this is the interpolant of
    kzg_verify_coset. Returns 2^lbits x 32 B Montgomery. device=None computes on the host."""
    handle = None if device is None else _context(device).handle
    return _coset_interp_fold(handle, nbits, lbits, index, ys_mont, weights_mont)


def _kzg_recover_cosets(handle, nbits, lbits, index, ys_mont, length, evals):
    index = list(index)
    count = len(index)
    ok = 0 <= nbits <= 23 and 0 <= lbits <= nbits  # else the library refuses before it reads or writes
    if ok and len(ys_mont) != (32 << lbits) * count:
        raise ValueError("ys_mont holds len(index) * 2^lbits 32-byte elements")
    idx = (ctypes.c_uint64 * max(count, 1))(*index)
    fits = ok and 1 <= length <= 1 << nbits
    coef = ctypes.create_string_buffer(32 * length if fits else 32)
    ev = ctypes.create_string_buffer(32 << nbits if ok else 32) if evals else None
    py, ky = _ptr(ys_mont) if len(ys_mont) else (None, None)  # read in place
    rc = _check(lib().kgs_kzg_recover_cosets(handle, nbits, lbits, ctypes.cast(idx, ctypes.c_void_p), py, count, length,
                                             coef, ev))
    del ky
    return (rc == 1, coef.raw, ev.raw) if evals else (rc == 1, coef.raw)


def kzg_recover_cosets(nbits, lbits, index, ys_mont, length, evals=False, device=0):
    """The polynomial of degree < length through the given cosets of the domain of 2^nbits points
    (kgs_kzg_recover_cosets): index holds distinct coset indices < m = 2^(nbits - lbits), in any order, and row k of
    ys_mont the 2^lbits Montgomery values p(w^(index[k] + m j)), as kzg_open_cosets' evaluations give them;
    len(index) * 2^lbits >= length. Returns (ok, coefs) or with evals=True (ok, coefs, evals): length x 32 B
    Montgomery coefficients and p(w^k) in natural order. ok is False when the values lie on no polynomial of
    degree < length; the other results then mean nothing. Needs no SRS."""
    return _kzg_recover_cosets(_context(device).handle, nbits, lbits, index, ys_mont, length, evals)


def _kzg_recover_cosets_many(handle, nbits, lbits, poly_of, index, ys_mont, length, polys, evals, stride, coefs_out):
    poly_of, index = list(poly_of), list(index)
    count = len(index)
    if len(poly_of) != count:
        raise ValueError("poly_of and index hold one entry per cell")
    ok = 0 <= nbits <= 23 and 0 <= lbits <= nbits  # else the library refuses before it reads or writes
    if ok and len(ys_mont) != (32 << lbits) * count:
        raise ValueError("ys_mont holds len(index) * 2^lbits 32-byte elements")
    stride = length if stride is None else stride
    fits = ok and 1 <= length <= 1 << nbits and stride >= length and 0 <= polys << nbits <= 1 << 24
    if coefs_out is None:
        coef = ctypes.create_string_buffer(max(32 * stride * polys, 32) if fits else 32)
        pcoef, kcoef = coef, None
    else:
        if not fits or len(coefs_out) != 32 * stride * polys:
            raise ValueError("coefs_out holds polys * stride 32-byte elements")
        pcoef, kcoef = _ptr(coefs_out)
    ev = ctypes.create_string_buffer(max((32 << nbits) * polys, 32) if fits else 32) if evals else None
    status = ctypes.create_string_buffer(max(polys, 1) if fits else 1)
    po = (ctypes.c_uint32 * max(count, 1))(*poly_of)
    idx = (ctypes.c_uint64 * max(count, 1))(*index)
    py, ky = _ptr(ys_mont) if len(ys_mont) else (None, None)  # read in place
    _check(lib().kgs_kzg_recover_cosets_many(handle, nbits, lbits, polys, ctypes.cast(po, ctypes.c_void_p),
                                             ctypes.cast(idx, ctypes.c_void_p), py, count, length, stride, pcoef, ev,
                                             status))
    del ky, kcoef
    out = bytes(coefs_out) if coefs_out is not None else coef.raw[:32 * stride * polys]
    return list(status.raw[:polys]), out, (ev.raw[:(32 << nbits) * polys] if evals else None)


def kzg_recover_cosets_many(nbits, lbits, poly_of, index, ys_mont, length, polys, evals=False, device=0):
    """kzg_recover_cosets for `polys` polynomials of `length` coefficients in one call (kgs_kzg_recover_cosets_many).
    The cells come as the batch verifier takes them: cell k belongs to polynomial poly_of[k] < polys, names coset
    index[k] < m = 2^(nbits - lbits), and row k of ys_mont holds its 2^lbits Montgomery values; any order, every
    polynomial its own set of cosets. Returns (status, coefs, evals): one status per polynomial (1 recovered, 0 its
    cells lie on no polynomial of degree < length, 2 fewer than ceil(length / 2^lbits) cells), polys x length x 32 B
    Montgomery coefficients, polynomial after polynomial, and with evals=True polys x 2^nbits x 32 B values in natural
    order (else None). The bytes of a polynomial with status 0 or 2 mean nothing. Needs no SRS."""
    return _kzg_recover_cosets_many(_context(device).handle, nbits, lbits, poly_of, index, ys_mont, length, polys, evals,
                                    None, None)


def grandsum_verifier(pTauFilename, proof, nBits):
    """mset_eq_kzg_grandsum_verifier (src/grandsum/mset_eq_kzg_verifier.js:9)."""
    return _verifier(GRANDSUM, pTauFilename, proof, nBits)


def grandproduct_verifier(pTauFilename, proof, nBits):
    """mset_eq_kzg_grandproduct_verifier (src/grandproduct/mset_eq_kzg_verifier.js:9)."""
    return _verifier(GRANDPRODUCT, pTauFilename, proof, nBits)


def lookup_prover(pTauFilename, evalsFs, evalsTs, evalsSelF=None, evalsMulT=None, device=0):
    """Lookup argument: every selected f row (evalsSelF, binary; all ones if None)
    is a row of the table t, and evalsMulT (Montgomery, required) holds how often each table row is
    looked up. The commented-out cases of test/lookup_kzg_grandsum.test.js:24-44 call the grand-sum
    prover with these arguments; this is that prover without the binary constraint on the
    multiplicities (include/kgs.h KGS_LOOKUP). Same proof layout as a selected grand-sum."""
    try:
        return _prover(LOOKUP, pTauFilename, evalsFs, evalsTs, evalsSelF, evalsMulT, device)
    except KgsError as e:
        raise _semantic(e) from e


def _lookup_lengths(evalsFs, evalsTs, evalsSelF):
    """_prover's list / length checks (same messages) for the calls that take no multiplicities."""
    if not isinstance(evalsFs, (list, tuple)):
        evalsFs = [evalsFs]
    if not isinstance(evalsTs, (list, tuple)):
        evalsTs = [evalsTs]
    if len(evalsFs) != len(evalsTs):
        raise ValueError("The lengths of the two vector multisets must be the same.")
    npols = len(evalsFs)
    if npols == 0:
        raise ValueError("The number of multisets must be greater than 0.")
    for i in range(npols):
        if evalsFs[i].length() != evalsTs[i].length():
            raise ValueError(f"The {i}-th multiset buffers must have the same length.")
        elif evalsFs[i].length() != evalsFs[0].length():
            raise ValueError("The multiset buffers must all have the same length.")
    if evalsSelF is not None and evalsSelF.length() != evalsFs[0].length():
        raise ValueError("The selection buffers must have the same length as the multiset buffers.")
    return evalsFs, evalsTs


def lookup_multiplicities(evalsFs, evalsTs, evalsSelF=None, device=0):
    """The evalsMulT of lookup_prover, computed on the GPU (include/kgs.h kgs_lookup_multiplicities): for
    every row of the table evalsTs, how many rows of evalsFs selected by evalsSelF (Montgomery zero /
    one; all rows if None) equal it. evalsFs / evalsTs are standard-form Evaluations (one, or a list of
    k columns) and are not modified. A table row that occurs several times gets all of its count at its
    first occurrence. Raises ValueError "Row <i> of F is not in the table." for the lowest selected row
    without a match."""
    evalsFs, evalsTs = _lookup_lengths(evalsFs, evalsTs, evalsSelF)
    if evalsFs[0].length() == 0:
        raise ValueError("The multiset buffers must not be empty.")
    try:
        m = _context(device).lookup_multiplicities([e.eval for e in evalsFs], [e.eval for e in evalsTs],
                                                   evalsSelF.eval if evalsSelF is not None else None)
    except KgsError as e:
        raise _semantic(e) from e
    out = Evaluations(b"")
    out.eval = m
    return out


def lookup_prover_from_table(pTauFilename, evalsFs, evalsTs, evalsSelF=None, device=0):
    """lookup_prover with the multiplicities computed from the table (lookup_multiplicities): the caller
    passes the witness, the table and, optionally, the selector of the witness rows."""
    evalsMulT = lookup_multiplicities(evalsFs, evalsTs, evalsSelF, device)
    return lookup_prover(pTauFilename, evalsFs, evalsTs, evalsSelF, evalsMulT, device)


def lookup_verifier(pTauFilename, proof, nBits):
    """Verifier of lookup_prover's proofs: the grand-sum verifier (src/grandsum/mset_eq_kzg_verifier.js:9)
    without the selT-binary term of r0 (:80-81)."""
    return _verifier(LOOKUP, pTauFilename, proof, nBits)


def _multi_arg(a):
    """One argument of multi_prover: a dict {"kind", "evalsFs", "evalsTs", "evalsSelF", "evalsSelT"} (the
    selectors optional; a lookup's multiplicities go in "evalsSelT") or the same as a tuple."""
    if isinstance(a, dict):
        return a["kind"], a["evalsFs"], a["evalsTs"], a.get("evalsSelF"), a.get("evalsSelT")
    a = tuple(a)
    return a + (None,) * (5 - len(a))


def multi_prover(pTauFilename, args, device=0):
    """One proof of several arguments over one domain (include/kgs.h kgs_prove_multi): the
    arguments share their challenges, one quotient and one pair of opening proofs. args: a list of 1 ..
    16 arguments (_multi_arg), each of kind GRANDSUM / GRANDPRODUCT / LOOKUP with the Evaluations the
    single provers take. Every argument passes the single provers' input checks (same messages, prefixed
    with "argument <j>: "). The inputs are left as they are (no Montgomery write-back). Returns the
    proof dict with the names of proof_names_multi."""
    log.info("> MULTI-ARGUMENT KZG PROVER STARTED")
    power = ptau_power(pTauFilename)
    args = [_multi_arg(a) for a in args]
    if not 1 <= len(args) <= MAX_ARGS:
        raise ValueError(f"The number of arguments must be in 1 .. {MAX_ARGS}.")
    recs, shapes, nbits = [], [], None
    for j, (kind, fs, ts, sf, st) in enumerate(args):
        if kind not in (GRANDSUM, GRANDPRODUCT, LOOKUP):
            raise ValueError(f"argument {j}: unknown argument kind")
        try:
            fs, ts, sf, st, selected, nb = _prover_inputs(kind, power, fs, ts, sf, st)
        except ValueError as e:
            raise ValueError(f"argument {j}: {e}") from None
        if nbits is not None and nb != nbits:
            raise ValueError(f"argument {j}: every argument must have the domain of argument 0.")
        nbits = nb
        recs.append((kind, [e.eval for e in fs], [e.eval for e in ts], sf.eval if selected else None,
                     st.eval if selected else None))
        shapes.append((kind, len(fs), selected))
    ctx = _context(device)
    ctx.load_ptau(pTauFilename, nbits)
    try:
        coms, evs = ctx.prove_multi(nbits, recs)
    except KgsError as e:
        raise _semantic(e) from e
    cn, en = proof_names_multi(shapes)
    log.info("> MULTI-ARGUMENT KZG PROVER FINISHED")
    return {"commitments": dict(zip(cn, coms)), "evaluations": dict(zip(en, evs))}


def multi_verifier(pTauFilename, proof, nBits, shapes):
    """Verifier of multi_prover's proofs (kgs_verify_multi_ptau; host only): shapes is the list of
    (kind, npols, selected) the proof was made for. False for a proof with a missing key or a value of the
    wrong length."""
    shapes = [tuple(s) for s in shapes]
    cn, en = proof_names_multi(shapes)
    try:
        com = b"".join(bytes(proof["commitments"][x]) for x in cn)
        ev = b"".join(bytes(proof["evaluations"][x]) for x in en)
    except KeyError:
        return False
    if len(com) != 64 * len(cn) or len(ev) != 32 * len(en):
        return False
    arr = (ArgShape * len(shapes))(*[ArgShape(k, p, 1 if s else 0) for k, p, s in shapes])
    rc = _check(lib().kgs_verify_multi_ptau(os.fsencode(pTauFilename), nBits, arr, len(shapes), _buf(com), _buf(ev)))
    return rc == 1
