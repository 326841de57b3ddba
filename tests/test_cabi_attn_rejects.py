"""CPU: what every sage_attn_* entry point refuses, and in which words.

Each case is a call that is valid but for ONE argument, built by parameter NAME from the header's prototype (test_cabi.prototypes), so that a
case reads as what it violates and applies to every entry point that has the parameter.  The library refuses all of them before its first HIP
call -- the tensors are host memory: a case that were accepted would be a launch on host pointers, so none may ever be.  SAGE_GFX950_LIB selects
the library; the table holds for the library as it was before the entry points shared one descriptor, which is what it was written against.

Two refusals the library has are no cases here because no C-ABI call can meet them: "V rows in place" with a split, a mask, a packed batch
or FP8 PV (no *_vrows prototype has kv_split, a mask or cu_seqlens, no *_split prototype has v strides), and "kv_split must divide the folded
kv-head count" (the split entries fold Hkv * kv_split heads themselves)."""
import ctypes

import pytest

import util  # noqa: F401  (sys.path)
from sageattention_amd import _cabi
from test_cabi import prototypes

ATTN = sorted(n for n in prototypes() if n.startswith("sage_attn_") and n != "sage_attn_launch_ws_bytes")
INT8_Q = [n for n in ATTN if "qk_int8" in n]                 # q INT8 with q_scale; every other entry quantises q (fp16 / bf16) itself
VARLEN = [n for n in ATTN if n.endswith("_varlen")]
FP8_VARLEN = [n for n in VARLEN if "pv_f8" in n]
SPLIT = ["sage_attn_fused_q_pv_f8_split", "sage_attn_fused_q_pv_f16_split"]
EXACT = "sage_attn_fused_q_pv_f8_split_exact"
KVLENS = "sage_attn_fused_q_pv_f8_kvlens"
VROWS = [n for n in ATTN if n.endswith("_vrows")]
QBLOCK_VARLEN = [n for n in VARLEN if "fused_qblock" in n]

_buf = ctypes.create_string_buffer(4096)
P = (ctypes.addressof(_buf) + 127) & ~127
FOLDED = "folded"            # stands for a SageLaunchAttr with SAGE_ATTR_FP8_FOLDED_SCORES

# a valid call: 1 sample (sequence), 4 query heads on 2 kv heads, 128 rows, 128 keys, head_dim 64, contiguous [B, H, L, D]; nullable arguments NULL
VALID = dict(B=1, nseq=1, Hq=4, Hkv=2, Lq=128, max_seqlen_q=128, Lk=128, Lk_chunk=64, D=64, kv_split=2, tail=0,
             q_sl=64, q_sh=64 * 128, q_sb=4 * 64 * 128, k_sl=64, k_sh=64 * 128, k_sb=2 * 64 * 128, v_sl=128, v_sh=128 * 128, v_sb=2 * 128 * 128,
             o_sl=64, o_sh=64 * 128, o_sb=4 * 64 * 128, m_sb=0, m_sh=0, m_sq=128, m_sk=1, lse_sh=128,
             is_causal=0, qk_quant_gran=_cabi.GRAN_PER_BLOCK, q_warp=32, pv_accum=_cabi.PV_ACCUM_TWO_LEVEL, out_dtype=_cabi.DTYPE_F16,
             q_dtype=_cabi.DTYPE_F16, mask_kind=_cabi.MASK_BOOL, items_bound=0, sm_scale_log2=1.0, q_premul=1.0,
             lse=None, v_mean=None, seq_order=None, work_items=None, work_hdr=None, stream=None, attr=None)


# the smallest k row stride (a multiple of 16) whose 64-key tile no longer fits an int offset at head_dim 64: 63 k_sl + 64 - 16 >= 2^31
K_SL_REFUSED = -(-((1 << 31) - 48) // 63 // 16) * 16
assert K_SL_REFUSED == 34087056 and 63 * (K_SL_REFUSED - 16) + 48 < 1 << 31 <= 63 * K_SL_REFUSED + 48


def all_but(*names):
    return [n for n in ATTN if n not in names]


# (case, entry points, the one argument that is wrong, a piece of the message)
CASES = [
    # ---- the checks every Q form shares
    ("null tensor", ATTN, dict(k=None), b"null tensor pointer"),
    ("null output", all_but(*SPLIT, EXACT), dict(o=None), b"null tensor pointer"),
    ("head_dim 96", ATTN, dict(D=96), b"head_dim must be 64 or 128 (got 96)"),
    ("empty problem", ATTN, dict(Hq=0), b"empty problem"),
    ("Hq % Hkv", all_but(*SPLIT), dict(Hq=3), b"num_qo_heads (3) must be divisible by num_kv_heads (2)"),
    ("Hq % Hkv, heads folded", SPLIT, dict(Hq=3), b"num_qo_heads (6) must be divisible by num_kv_heads (4)"),
    ("out dtype code", all_but(EXACT), dict(out_dtype=7), b"bad out_dtype 7"),
    ("misaligned q", all_but(EXACT), dict(q=P + 2), b"q/k/v/o must be 16-byte aligned"),
    ("misaligned o", all_but(*SPLIT, EXACT), dict(o=P + 8), b"q/k/v/o must be 16-byte aligned"),
    ("k stride", INT8_Q, dict(k_sl=72), b"int8 q/k strides must be multiples of 16"),
    ("k stride", all_but(*INT8_Q), dict(k_sh=64 * 128 + 8), b"int8 k strides must be multiples of 16"),
    # (the kernels form a lane's offset into a 64-key tile as int: 63 k_sl + D - 16 < 2^31.  At D 64 the largest stride of whole 16-byte units that
    #  passes is 34087040; the next one, and a stride that (int) would truncate to 0)
    ("k tile, the first stride refused", ATTN, dict(k_sl=K_SL_REFUSED), b"one 64-key tile of k must span less than 2 GiB (row stride 34087056)"),
    ("k tile, a stride of 2^31", ATTN, dict(k_sl=1 << 31), b"one 64-key tile of k must span less than 2 GiB (row stride 2147483648)"),
    ("o stride", all_but(EXACT), dict(o_sl=68), b"output strides must be multiples of 8 elements"),
    # ---- per Q form
    ("q stride, INT8", INT8_Q, dict(q_sl=72), b"int8 q/k strides must be multiples of 16"),
    ("q stride, fp16", all_but(*INT8_Q), dict(q_sl=68), b"q strides must be multiples of 8 elements"),
    ("q dtype code", [n for n in all_but(*INT8_Q) if n not in VROWS], dict(q_dtype=2), b"bad q_dtype 2"),
    ("null q_scale", INT8_Q, dict(q_scale=None), b"null tensor pointer"),
    ("granularity", ["sage_attn_qk_int8_pv_f8", "sage_attn_qk_int8_pv_f16", "sage_attn_qk_int8_pv_f16_vrows"], dict(qk_quant_gran=4), b"bad qk_quant_gran 4"),
    ("q_warp", ["sage_attn_qk_int8_pv_f8", "sage_attn_qk_int8_pv_f16", "sage_attn_qk_int8_pv_f16_vrows"], dict(qk_quant_gran=_cabi.GRAN_PER_WARP, q_warp=64),
     b"per_warp q_warp must be 32 or 16 (got 64)"),
    ("pv_accum", ["sage_attn_qk_int8_pv_f8", "sage_attn_qk_int8_pv_f8_varlen", "sage_attn_fused_qblock_pv_f8_varlen"], dict(pv_accum=_cabi.PV_ACCUM_TRITON), b"bad pv_accum 2"),
    ("pv_accum", ["sage_attn_qk_int8_pv_f16", "sage_attn_qk_int8_pv_f16_vrows", "sage_attn_qk_int8_pv_f16_varlen"], dict(pv_accum=3), b"bad pv_accum 3"),
    ("FP8 PV without v_scale", ["sage_attn_qk_int8_pv_f8", "sage_attn_qk_int8_pv_f8_varlen", "sage_attn_fused_qblock_pv_f8_varlen"], dict(v_scale=None), b"fp8 PV needs v_scale"),
    ("FP8 PV without v_scale", ["sage_attn_fused_q_pv_f8", "sage_attn_fused_q_pv_f8_split", KVLENS, EXACT], dict(v_scale=None), b"null tensor pointer"),
    ("no keys", ["sage_attn_qk_int8_pv_f8", "sage_attn_qk_int8_pv_f16", "sage_attn_qk_int8_pv_f16_vrows", "sage_attn_qk_int8_pv_f16_masked"], dict(Lk=0), b"kv_len must be positive"),
    ("no keys", [n for n in all_but(*INT8_Q, *VARLEN, *SPLIT)], dict(Lk=0), b"empty problem"),
    # ---- masks
    ("mask pointer", ["sage_attn_qk_int8_pv_f16_masked"], dict(mask=None), b"null attn_mask pointer"),
    ("mask kind", ["sage_attn_qk_int8_pv_f16_masked"], dict(mask_kind=4), b"bad mask_kind 4"),
    # ---- V rows in place
    ("v stride", VROWS, dict(v_sh=128 * 128 + 4), b"v strides must be multiples of 8 elements (16-byte rows)"),
    ("v rows shorter than head_dim", VROWS, dict(v_sl=56), b"v strides must be multiples of 8 elements (16-byte rows)"),
    ("a head of v of 2 GiB", VROWS, dict(v_sl=1 << 24), b"one head of v must span less than 2 GiB"),
    # ---- packed batches and their work list
    ("prefix arrays", VARLEN, dict(cu_seqlens_k=None), b"varlen needs cu_seqlens"),
    ("per-block Q without cu_seqlens_q", QBLOCK_VARLEN, dict(cu_seqlens_q=None), b"varlen needs cu_seqlens_q"),
    ("work list without header", VARLEN, dict(work_items=P, items_bound=4), b"the work list comes as (work_items, work_hdr, items_bound > 0), varlen only"),
    ("work list without bound", VARLEN, dict(work_items=P, work_hdr=P), b"the work list comes as (work_items, work_hdr, items_bound > 0), varlen only"),
    ("packed FP8, folded scores", FP8_VARLEN, dict(attr=FOLDED), b"packed (varlen) FP8 attention has the exact score form only"),
    ("packed lse without its stride", FP8_VARLEN, dict(lse=P, lse_sh=0), b"its head stride lse_sh must be positive (got 0)"),
    # ---- per-sample key lengths
    ("kv_lens, folded scores", [KVLENS], dict(attr=FOLDED), b"kv_lens: FP8 PV, the exact score form"),
    ("null kv_lens", [KVLENS], dict(kv_lens=None), b"null kv_lens"),
    # ---- the splits
    ("one chunk", SPLIT, dict(kv_split=1), b"kv_split must be at least 2 (got 1)"),
    ("partial buffers", SPLIT, dict(lse_part=None), b"split-KV needs the partial output and log-sum-exp buffers"),
    ("ragged chunk", SPLIT, dict(Lk_chunk=100), b"split-KV chunks are whole numbers of 64-key tiles (got 100 keys)"),
    ("kv_split not dividing", [EXACT], dict(kv_split=3, Lk=256), b"kv_split (3) must divide the number of whole 64-key tiles (256 keys: 4 tiles)"),
    ("tail without ragged keys", [EXACT], dict(tail=1), b"tail = 1 needs a ragged key range (Lk = 128 is a multiple of 64)"),
    ("tail code", [EXACT], dict(tail=2), b"tail must be 0 (the whole chunks) or 1 (the ragged tail), got 2"),
    ("exact split, folded scores", [EXACT], dict(attr=FOLDED), b"the exact split takes the exact score form only"),
    ("exact split buffers", [EXACT], dict(chunk_max=None), b"null tensor pointer"),
    ("exact split, misaligned q", [EXACT], dict(q=P + 2), b"q/k must be 16-byte aligned"),
    ("exact split, misaligned partials", [EXACT], dict(o_part=P + 4), b"v_image / o_part must be 16-byte aligned"),
]


def _cases():
    for what, entries, wrong, msg in CASES:
        for name in entries:
            yield pytest.param(name, wrong, msg, id=f"{name[len('sage_attn_'):]}-{what.replace(' ', '_')}")


@pytest.mark.parametrize("name, wrong, msg", list(_cases()))
def test_attention_entry_refuses(name, wrong, msg):
    params = prototypes()[name][1]
    names = [pname for _, pname in params]
    assert set(wrong) <= set(names), f"{name} has no parameter {sorted(set(wrong) - set(names))}"
    folded = _cabi.SageLaunchAttr(struct_bytes=ctypes.sizeof(_cabi.SageLaunchAttr), flags=_cabi.ATTR_FP8_FOLDED_SCORES)
    args = []
    for ctype, pname in params:
        v = wrong[pname] if pname in wrong else VALID[pname] if pname in VALID else P
        assert pname in wrong or pname in VALID or ctype.endswith("*"), f"{name}: no valid value for {ctype} {pname}"
        args.append(ctypes.byref(folded) if v is FOLDED else v)
    lib = _cabi.load()
    rc = getattr(lib, name)(*args)
    assert rc == -1 and msg in lib.sage_last_error(), (rc, lib.sage_last_error())


def test_every_attention_entry_has_every_shared_case():
    """the shared checks are asked of all 17 entry points (an entry point added later joins ATTN by its name and so joins the table)"""
    assert len(ATTN) == 17            # a deliberate tripwire: a new attention entry point comes with a look at the table's entry lists
    covered = {}
    for what, entries, _, _ in CASES:
        for name in entries:
            covered.setdefault(name, set()).add(what.split(",")[0])
    for name in ATTN:
        need = {"null tensor", "head_dim 96", "Hq % Hkv", "misaligned q" if name != EXACT else "exact split", "k stride", "k tile", "q stride", "empty problem"}
        need.add("q dtype code" if name == EXACT else "out dtype code")
        assert need <= covered[name], f"{name}: no case for {sorted(need - covered[name])}"
