"""What bounds the e2m3 MX GEMM: side builds of gemm_mx.hip that change one thing each, against the in-tree build --
  BYA_MX_E2M3_STAGES = 2 / 3: LDS ring depth (two stages: every K-tile waits for all its loads; three: a counted wait keeps
  the next K-tile's DMA in flight across the barrier) -- i.e. does DMA latency bound it;
  BYA_MX_E2M3_BIG_TILE = 0 / 1: 128 x 128 tiles (4 waves, two or three workgroups per CU) or 256 x 256 tiles (8 waves, one
  per CU) for launches of >= 200 such tiles -- half the L2 -> LDS bytes per FLOP, i.e. does that traffic bound it.
Times bya_gemm_mx (mxfp6, and mxfp8 which none of the switches touch) at the four DiT Linear shapes (17776 rows) in a fresh
child process per library.  Only the time is read (the builds differ in summation order at most).
usage: python tools/mx_ring_ablate.py [out.json]     (needs the in-tree build: python __graft_entry__.py)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("qkv", 9216, 3072), ("attn_out", 3072, 3072), ("ff1", 12288, 3072), ("ff2", 3072, 12288)]


VARIANTS = {"e2m3_128_two_stages": ["-DBYA_MX_E2M3_STAGES=2", "-DBYA_MX_E2M3_BIG_TILE=0"],
            "e2m3_128_three_stages": ["-DBYA_MX_E2M3_STAGES=3", "-DBYA_MX_E2M3_BIG_TILE=0"],
            "e2m3_256_three_stages": ["-DBYA_MX_E2M3_STAGES=3", "-DBYA_MX_E2M3_BIG_TILE=1"]}     # (in-tree: 256 x 256, two stages)


def side_build(name, defines):
    from bind_your_avatar_implementation_amd import build as B
    out_dir = os.path.join(B.PKG_DIR, "build", "mx_ablate_" + name)
    os.makedirs(out_dir, exist_ok=True)
    hipcc = B._hipcc()
    obj = os.path.join(out_dir, "gemm_mx.o")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-mllvm",
                           "-amdgpu-mfma-vgpr-form=1", "-fno-slp-vectorize", *defines, "-c",
                           os.path.join(B.CSRC, "gemm_mx.hip"), "-o", obj])
    objs = [os.path.join(B.PKG_DIR, "build", s.replace(".hip", ".o")) for s in B.SOURCES if s != "gemm_mx.hip"]
    lib = os.path.join(out_dir, "libbya_hip.so")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs + [obj, "-ldl"])
    return lib


def child():
    import torch
    from bind_your_avatar_implementation_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    res = {}
    for name, N, K in SHAPES:
        M = 17776
        a = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
        w = (torch.randn(N, K, device=dev, generator=g) * K ** -0.5).to(torch.bfloat16)
        c = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        for f in ("mxfp6", "mxfp8"):
            (ac, asc), (wc, wsc) = ops.quantize_mx(a, f), ops.quantize_mx(w, f)
            best = 1e30
            for _ in range(3):
                ops.gemm_mx(ac, asc, wc, wsc, c, f)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(10):
                    ops.gemm_mx(ac, asc, wc, wsc, c, f)
                e1.record()
                torch.cuda.synchronize()
                best = min(best, e0.elapsed_time(e1) / 10 * 1e3)
            res[f"{name}:{f}"] = {"us": round(best, 1), "tflops": round(2.0 * M * N * K / best * 1e-6, 1)}
    print(json.dumps(res), flush=True)


def main():
    if "--child" in sys.argv:
        return child()
    libs = {"in-tree (e2m3_256_two_stages)": None}
    libs.update({name: side_build(name, d) for name, d in VARIANTS.items()})
    out = {}
    for label, lib in libs.items():
        env = dict(os.environ)
        if lib:
            env["BYA_HIP_LIB"] = lib
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True,
                           timeout=300)
        if r.returncode != 0:
            raise SystemExit(f"{label}: child exited {r.returncode}\n{r.stderr[-2000:]}")
        out[label] = json.loads(r.stdout.strip().splitlines()[-1])
        print(label, json.dumps(out[label]), flush=True)
    path = next((a for a in sys.argv[1:] if not a.startswith("--")), None)
    if path:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
