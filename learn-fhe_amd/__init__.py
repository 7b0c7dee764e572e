"""learn-fhe_amd: MI355X (gfx950) polynomial-ring backend for the FHE hot path of han0110/learn-fhe.

The product is the C-ABI shared library `lib/libfhe_ring.so` (include/fhe_ring.h) built from the HIP
sources in `csrc/`.  This Python package is only the harness-side binding used by tests and bench:
it loads the library with ctypes and fails loudly if it is missing -- there is no CPU fallback.
"""
from ._lib import FheError, build, lib, lib_path, set_option  # noqa: F401
from . import circuit  # noqa: F401
from . import ckks_poly  # noqa: F401
from .ckks_poly import CkksPolyEval, CkksPolyPlan, eval_mod_plan  # noqa: F401
from . import ckks_bootstrap  # noqa: F401
from .ckks_bootstrap import CkksBootstrapper, bootstrap_eval_mod_plan, cjk_gen  # noqa: F401
from .circuit import Circuit  # noqa: F401
from . import tfhe_circuit  # noqa: F401
from . import tfhe_cbs  # noqa: F401
from .tfhe_cbs import lut_eval_batch, lut_eval_batch_steps, lut_pack, lut_shape  # noqa: F401
from . import tfhe_wop  # noqa: F401
from .tfhe_wop import wop_pbs, wop_selectors, wop_table  # noqa: F401
from . import tfhe_pack  # noqa: F401
from .tfhe_pack import PackKey, pack, pack_composed, pack_funcs  # noqa: F401
from . import tfhe_mul  # noqa: F401
from .tfhe_mul import RelinKey, rlk_gen  # noqa: F401
from . import tfhe_trace  # noqa: F401
from .tfhe_trace import AutoKey, atk_gen, galois_set, ring_pack  # noqa: F401
from . import ckks_hoist  # noqa: F401
from .ckks_hoist import extend_plain, mul_mat_hoisted_composed, rotate_many_composed  # noqa: F401
from .ring import (BootstrapKey, CkksDiagMatrix, CkksDiagMatrixHoisted, CkksEncoder, CkksKey, CkksLinearPlan, CkksLinearTransform, CkksShard, Fhew, GadgetKey, NttContext, RnsContext, TggswKey, TorusContext,  # noqa: F401
                   ak_t, automorphism, bsgs_split, decompose, lwe_key_switch, lwe_lincomb, lwe_mod_switch, monomial_mul, rlwe_sample_extract, rq_add, rq_from_i64, rq_neg, rq_scalar_mul, rq_sub,
                   tglwe_sample_extract, tglwe_sample_extract_many, tlwe_key_switch, tlwe_lincomb, torus_decompose, tglwe_rotate,
                   power_up, rgsw_encrypt, rlwe_ksk_gen, rlwe_sk_encrypt, sample_dg, sample_torus, sample_uniform,
                   lwe_ksk_gen, lwe_sk_encrypt, rq_sum,
                   sample_binary, sample_tdg, sample_zo, tggsw_encrypt, tglwe_sk_encrypt, tlwe_ksk_gen, tlwe_sk_encrypt,
                   rlwe_share_encrypt, rlwe_pk_encrypt, rlwe_decrypt, rgsw_pk_encrypt, lwe_share_encrypt, lwe_ksk_share_gen,
                   TggswKeyK, tglwek_rotate, tglwek_sample_extract, tglwek_sk_encrypt, tggswk_encrypt,
                   TGGSWK_FORM_COMPOSED, TGGSWK_FORM_X3, tggswk_form_for,
                   rtk_gen,
                   Rng, STREAM_AUTO, chacha20_block)
