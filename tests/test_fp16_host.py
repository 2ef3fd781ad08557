"""CPU-only tests of the fp16 model path (`-m "not gpu"`): the dtype code on both sides of the C ABI, the ABI version,
the generated gfx950 ISA of the fp16 GEMM and attention instantiations (device-only compile, no GPU needed), and the
wrapper's argument checks that need no device."""
import os
import re
import subprocess
import sys

import pytest
import torch

import rajni_amd
from rajni_amd import _native as nat, timm_shaped as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rajni-vit_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def test_dtype_code_float16_matches_header():
    with open(os.path.join(ROOT, "include", "rajni_hip.h")) as f:
        m = re.search(r"RAJNI_F16\s*=\s*(\d+)", f.read())
    assert m is not None, "RAJNI_F16 missing from the dtype enum"
    assert nat.dtype_code(torch.float16) == nat.RAJNI_F16 == int(m.group(1)) == 2
    assert nat.dtype_code(torch.bfloat16) == nat.RAJNI_BF16 == 1
    assert nat.dtype_code(torch.float32) == nat.RAJNI_F32 == 0


def test_abi_version_unchanged():
    assert nat.load_library().rajni_abi_version() == nat.ABI_VERSION == 8


def _functions(asm):
    """mangled kernel name -> its instruction text"""
    out, name, body = {}, None, []
    for line in asm.splitlines():
        m = re.match(r"^(_Z\S+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is not None:
            body.append(line)
            if line.startswith(".Lfunc_end"):
                out[name] = "\n".join(body)
                name = None
    return out


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("isa")
    res = {}
    for src in ("gemm.hip", "attention.hip"):
        out = tmp / (src + ".s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        os.path.join(CSRC, src), "-o", str(out)], check=True, capture_output=True, timeout=900)
        res[src] = _functions(out.read_text())
    return res


@needs_hipcc
def test_f16_gemm_instantiations_issue_f16_mfma(isa):
    f16 = {k: v for k, v in isa["gemm.hip"].items() if re.search(r"gemm_bf16_tn_(stream|128x128)I.*DF16_", k)}
    assert len(f16) >= 12, sorted(f16)
    for name, body in f16.items():
        assert re.search(r"v_mfma_f32_\d+x\d+x\d+_f16", body), f"{name}: no f16 MFMA"
        assert "_bf16" not in " ".join(re.findall(r"v_mfma\S*", body)), f"{name}: bf16 MFMA in an fp16 kernel"
        assert "pkrtz" not in body, f"{name}: round-toward-zero conversion"
    bf16 = [k for k in isa["gemm.hip"] if re.search(r"gemm_bf16_tn_(stream|128x128)I", k) and "DF16_" not in k]
    for name in bf16:
        assert "_f16 " not in isa["gemm.hip"][name], f"{name}: f16 MFMA in a bf16 kernel"


@needs_hipcc
def test_f16_attention_instantiations_issue_f16_mfma(isa):
    f16 = {k: v for k, v in isa["attention.hip"].items() if "attn_bf16_" in k and "DF16_" in k}
    assert len(f16) >= 10, sorted(f16)
    kinds = set()
    for name, body in f16.items():
        ops = re.findall(r"v_mfma\S*", body)
        assert ops and all(o.endswith("_f16") for o in ops), f"{name}: {sorted(set(ops))}"
        assert "pkrtz" not in body, f"{name}: round-toward-zero conversion"
        kinds.add(re.search(r"attn_bf16_(d64_stream|d64_full|dgen|d64)", name).group(1))
    assert kinds == {"d64", "d64_full", "d64_stream", "dgen"}, kinds
    assert any("attn_cls_kernelIDF16_" in k for k in isa["attention.hip"])


@needs_hipcc
def test_f16_gemm_isa_has_no_dma_drain_or_spill():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scan_isa.py")], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    f16 = [l for l in r.stdout.splitlines() if " f16 " in l]
    assert len(f16) >= 12 and all(l.endswith(" ok") for l in f16), "\n".join(f16)
    assert sum("dispatched  ok" in l for l in f16) >= 12


def test_set_residual_dtype_argument_check():
    cfg = ts.CONFIGS["vit_micro_patch16_64"]
    model = ts.create_model(cfg, seed=0, std=0.08, bias_std=0.02, round_bf16=True)
    w = rajni_amd.RAJNIViTWrapper(model, {1: {"keep_ratio": 0.75, "update": True}})
    assert w.set_residual_dtype(torch.float16) is w
    w.set_residual_dtype(torch.bfloat16)
    w.set_residual_dtype(torch.float32)
    for bad in (torch.float64, torch.int8, "float16"):
        with pytest.raises(ValueError, match="torch.float16"):
            w.set_residual_dtype(bad)
