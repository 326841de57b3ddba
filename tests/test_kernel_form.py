"""tools/kernel_form.py against csrc/sage_attn_form.h: the helper the build tests read kernel names with decodes every form of every unit's
list to the fields the header packs, and refuses what is not a kernel's name.  No GPU needed: a small host program prints the lists."""
import os
import subprocess

import pytest

import test_build_resources as tbr

kf = tbr.kf
CSRC = os.path.join(tbr.ROOT, "sageattention_amd", "csrc")
FIELDS = ("pv_fp8", "causal", "kthread", "two_level", "mask", "qf", "gpack", "sfold", "cpers", "vrows", "seed", "window", "qstart", "kvlen")
# the units in the order of the header's SAGE_ATTN_UNITS, as the files are named
UNITS = ("f8", "f8f", "f16", "f8v", "f8vb", "f8vbw", "f8s", "f8k", "f8q", "f8w", "f8g", "f8ks")
COUNTS = dict(f8=12, f8f=12, f16=33, f8v=12, f8vb=4, f8vbw=4, f8s=4, f8k=4, f8q=2, f8w=2, f8g=8, f8ks=8)
PROGRAM = r"""
#include "sage_attn_form.h"
#include <cstdio>
using namespace sage;
int main()
{
    for (int u = 0; u < UNIT_COUNT; u++)
        for (int D : {128, 64}) {
            const FormList l = unit_forms((AttnUnit)u, D);
            for (int i = 0; i < l.n; i++) {
                const AttnForm f = unpack(l.v[i]);
                printf("%d %u %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", u, l.v[i], f.D, f.pv_fp8, f.causal, f.kthread, f.two_level, f.mask, f.qf,
                       f.gpack, f.sfold, f.cpers, f.vrows, f.seed, f.window, f.qstart, f.kvlen);
            }
        }
    return UNIT_COUNT;
}
"""


@pytest.fixture(scope="module")
def listed(tmp_path_factory):
    """[(unit, packed form, the fields as the header unpacks them)] of every list"""
    tmp = tmp_path_factory.mktemp("forms")
    src, exe = tmp / "forms.hip", tmp / "forms"
    src.write_text(PROGRAM)
    out = subprocess.run([tbr.HIPCC, "-std=c++17", "--cuda-host-only", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == len(UNITS), (run.returncode, run.stderr)
    rows = []
    for line in run.stdout.split("\n"):
        if line:
            w = [int(x) for x in line.split()]
            f = {"D": w[2], **{k: (v if k in ("mask", "qf") else bool(v)) for k, v in zip(FIELDS, w[3:])}}
            rows.append((UNITS[w[0]], w[1], f))
    return rows


@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_every_listed_form_round_trips(listed):
    assert len(listed) == 2 * sum(COUNTS.values()) and len({w for _, w, _ in listed}) == len(listed)        # (no form in two lists)
    for d in (128, 64):
        assert {u: sum(1 for v, _, f in listed if v == u and f["D"] == d) for u in UNITS} == COUNTS
    assert set(kf.fields()[0]) == {"d128", *FIELDS}
    for unit, word, f in listed:
        assert kf.unpack(word) == f and kf.pack(f) == word, (unit, word, f)
        assert kf.decode(kf.encode(f)) == f and kf.encode(f) == f"_ZN4sage16sage_attn_kernelILj{word}EEEvNS_10AttnParamsE", (unit, word)
        assert kf.form(f["D"], **{k: v for k, v in f.items() if k != "D" and v}) == f
        assert kf.describe(f).split()[0] == f"D{f['D']}"


@pytest.mark.skipif(not os.path.exists(tbr.HIPCC), reason="hipcc not installed")
def test_a_compiled_unit_reports_the_names_of_its_list(listed):
    rep = tbr._resource_report("sage_attn_d64_f8q.hip")
    names = {k for k in rep if "sage_attn_kernel" in k}
    assert names == {kf.encode(f) for u, _, f in listed if u == "f8q" and f["D"] == 64} and len(names) == 2


def test_made_up_names_are_refused():
    good = kf.encode(kf.form(128, pv_fp8=True, causal=True, kthread=True, two_level=True, qf=1, kvlen=True))
    assert kf.decode(good)["kvlen"] and kf.decode(good)["D"] == 128
    nbits = kf.fields()[1]
    for bad in ("_ZN4sage16sage_attn_kernelILi128EEEvNS_10AttnParamsE",              # an int argument, not the unsigned form: not this kernel
                "_ZN4sage17prepass_kv_kernelILj3EEEvNS_10AttnParamsE", good + "x", good[1:], "",
                kf.encode(kf.form(64)).replace("ILj0E", f"ILj{1 << nbits}E"),        # a bit no field owns
                kf.encode(kf.form(64)).replace("ILj0E", f"ILj{5 << kf.fields()[0]['qf'][0]}E")):      # qf = 5
        with pytest.raises(ValueError):
            kf.decode(bad)
    for bad in (dict(qf=5), dict(mask=4)):
        with pytest.raises(ValueError):
            kf.pack(kf.form(64, **bad))
    with pytest.raises(ValueError):
        kf.form(64, colour=True)
    with pytest.raises(ValueError):
        kf.form(96)
