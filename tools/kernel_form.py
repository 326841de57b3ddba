"""Names of the attention kernels <-> their forms.

A member of the family is `sage::sage_attn_kernel<FORM>`: one unsigned template argument, the packed AttnForm of csrc/sage_attn_form.h.  The
compiler reports it as `_ZN4sage16sage_attn_kernelILj<FORM>EEEvNS_10AttnParamsE`.  The field positions are read from the header's FORM_*_POS /
FORM_*_LEN enumerators, so a flag added there is decoded here without an edit.  Used by the build tests and by tools/res_summary.py."""
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sageattention_amd", "csrc", "sage_attn_form.h")
_NAME = re.compile(r"^_ZN4sage16sage_attn_kernelILj(\d+)EEEvNS_10AttnParamsE$")
# a paged kernel is `sage::sage_attn_paged_kernel<FORM>`: the same form, its tiles reached through a block table (a second argument, no form bit)
_PAGED_NAME = re.compile(r"^_ZN4sage22sage_attn_paged_kernelILj(\d+)EEEvNS_10AttnParamsENS_9PagedArgsE$")
_INTS = ("mask", "qf")                    # every other field is a flag
_RANGE = {"mask": 3, "qf": 4}             # (form_error() of the header: the largest value of a field whose bits hold more)


def fields():
    """-> {field name: (lowest bit, bits)} and the number of bits in use, from the header"""
    text = open(HEADER).read()
    found = {m.group(1).lower(): (int(m.group(2)), int(m.group(3)))
             for m in re.finditer(r"\bFORM_(\w+)_POS\s*=\s*(\d+),\s*FORM_\1_LEN\s*=\s*(\d+)", text)}
    nbits = int(re.search(r"\bFORM_BITS\s*=\s*(\d+)", text).group(1))
    used = sorted(found.values())
    assert found and used[0][0] == 0 and all(a + n == b for (a, n), (b, _) in zip(used, used[1:])) and sum(used[-1]) == nbits, found
    return found, nbits


def form(D, **on):
    """The form of head size D with the named fields set and everything else off (FP16 PV says sfold=True)."""
    f = {"D": D, **{k: (0 if k in _INTS else False) for k in fields()[0] if k != "d128"}}
    unknown = set(on) - set(f)
    if unknown or D not in (64, 128):
        raise ValueError(f"not a form: D = {D}, unknown fields {sorted(unknown)}")
    f.update(on)
    return f


def unpack(word):
    """packed form -> {field: value}: D as 64 / 128, mask and qf as ints, the flags as bools"""
    layout, nbits = fields()
    if word < 0 or word >> nbits:
        raise ValueError(f"form {word:#x} has bits beyond the {nbits} the header defines")
    f = {}
    for k, (pos, n) in layout.items():
        val = word >> pos & ((1 << n) - 1)
        if val > _RANGE.get(k, (1 << n) - 1):
            raise ValueError(f"form {word:#x}: {k} = {val} is out of range")
        if k == "d128":
            f["D"] = 128 if val else 64
        else:
            f[k] = val if k in _INTS else bool(val)
    return f


def pack(f):
    layout = fields()[0]
    if set(f) != {"D"} | (set(layout) - {"d128"}) or f["D"] not in (64, 128):
        raise ValueError(f"not a form: {f}")
    word = 0
    for k, (pos, n) in layout.items():
        val = int(f["D"] == 128) if k == "d128" else int(f[k])
        if not 0 <= val <= _RANGE.get(k, (1 << n) - 1):
            raise ValueError(f"{k} = {val} is out of range")
        word |= val << pos
    return word


def decode(name):
    """reported kernel name -> form; ValueError on anything that is not an attention kernel's name"""
    m = _NAME.match(name)
    if not m:
        raise ValueError(f"not a name of sage_attn_kernel<FORM>: {name}")
    return unpack(int(m.group(1)))


def decode_paged(name):
    """reported name of a paged kernel -> its form; ValueError on anything else (decode() does not accept these names, nor this one those)"""
    m = _PAGED_NAME.match(name)
    if not m:
        raise ValueError(f"not a name of sage_attn_paged_kernel<FORM>: {name}")
    return unpack(int(m.group(1)))


def encode_paged(f):
    return f"_ZN4sage22sage_attn_paged_kernelILj{pack(f)}EEEvNS_10AttnParamsENS_9PagedArgsE"


def encode(f):
    return f"_ZN4sage16sage_attn_kernelILj{pack(f)}EEEvNS_10AttnParamsE"


def describe(f):
    """'D128 pv_fp8 causal qf=1 kvlen': the head size and what is on"""
    return " ".join([f"D{f['D']}"] + [k if v is True else f"{k}={v}" for k, v in f.items() if k != "D" and v])
