"""SHA-256 of every output of the four small-channel 3x3 convolutions (csrc/conv_small_n.hip, conv_rgb8.hip, conv_rgb_in.hip) over the cases their tests
run: the parameter lists of test_conv3x3_small_n and test_conv3x3_small_cin (tests/test_ops_gpu.py), SHAPES of tests/test_vae_rgb8_gpu.py and CONV_CASES
of tests/test_vae_encode_gpu.py, imported from those files.  One line per case: "<kernel> <case> <sha256> <bytes>"; every output lies in a guarded
buffer and the guards are part of what is hashed.  The inputs are seeded by the case names, so two trees that compute the same bytes print the same text:
    python tools/conv_small_digest.py > a.txt      (here)
    python tools/conv_small_digest.py > b.txt      (in a tree of the commit to compare with, built on its own)
    python tools/conv_small_digest.py --compare a.txt b.txt
--compare prints both columns side by side and the verdict; it needs no GPU.  Nothing is compared with a reference here: that is the tests' job."""
import argparse
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _params(fn):
    """the argument tuples of a test's parametrize mark"""
    (mark,) = [m for m in fn.pytestmark if m.name == "parametrize"]
    return [tuple(getattr(p, "values", p)) for p in mark.args[1]]


def _gen(name):
    import torch
    return torch.Generator().manual_seed(int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little"))


def _line(kernel, name, buf):
    import torch
    raw = buf.contiguous().view(torch.uint8).cpu().numpy().tobytes()
    return f"{kernel} {name} {hashlib.sha256(raw).hexdigest()} {len(raw)}"


def _conv(x, w, bias, corner, cin_valid):
    """mx_conv3x3 as ops.conv3x3 describes it, into a guarded buffer; returns the buffer"""
    import kernel_ref as R
    from sduss_amd import lib as L
    b, h, wd, cin = x.shape
    cout = w.shape[0]
    buf, view = R.guarded(b * h * wd, cout, cout, x.dtype, x.device)
    d = L.GemmDesc()
    d.a, d.w, d.c, d.bias = x.data_ptr(), w.data_ptr(), view.data_ptr(), bias.data_ptr()
    d.M, d.N, d.K, d.ldc, d.ldr, d.rows_per_batch = b * h * wd, cout, 9 * cin, cout, cout, h * wd
    d.B, d.Hin, d.Win, d.Cin, d.Hout, d.Wout, d.stride, d.up, d.corner_patch, d.cin_valid = b, h, wd, cin, h, wd, 1, 0, corner, cin_valid
    (kernel,) = L.gemm_kernels_of(d, conv=True)
    L.check(L.load().mx_conv3x3(L.current_stream(), C.byref(d)), "mx_conv3x3")
    return kernel, buf


def digest_lines():
    import torch
    import kernel_ref as R
    import test_ops_gpu as TO
    import test_vae_encode_gpu as TE
    import test_vae_rgb8_gpu as T8
    from sduss_amd import ops
    bf = torch.bfloat16
    for corner, h, w, cin, cout, b in _params(TO.test_conv3x3_small_n):
        name = f"corner{corner}-h{h}-w{w}-cin{cin}-cout{cout}-b{b}"
        g = _gen("small_n " + name)
        x = torch.randn(b, h, w, cin, generator=g).to(bf).cuda()
        wt = (torch.randn(cout, 9 * cin, generator=g) * (9 * cin) ** -0.5).to(bf).cuda()
        kernel, buf = _conv(x, wt, torch.randn(cout, generator=g).cuda(), corner, 0)
        assert kernel == "conv3x3_small_n_kernel", kernel
        yield _line(kernel, name, buf)
    for corner, h, w, cout, b, cv in _params(TO.test_conv3x3_small_cin):
        name = f"corner{corner}-h{h}-w{w}-cout{cout}-b{b}-cv{cv}"
        g = _gen("small_cin " + name)
        x = torch.zeros(b, h, w, 64)
        x[..., :cv] = torch.randn(b, h, w, cv, generator=g)
        wt = (torch.randn(cout, 9 * 64, generator=g) * (9 * cv) ** -0.5).to(bf).cuda()
        kernel, buf = _conv(x.to(bf).cuda(), wt, torch.randn(cout, generator=g).cuda(), corner, 8)
        assert kernel == "conv3x3_small_cin_kernel", kernel
        yield _line(kernel, name, buf)
    for p in T8.SHAPES:
        B, H, W, Cin = p.values
        g = _gen("rgb8 " + p.id)
        x = torch.randn(B, H, W, Cin, generator=g).to(bf).cuda()
        wt = torch.full((4, 9 * Cin), float("nan"), dtype=bf)
        wt[:3] = (torch.randn(3, 9 * Cin, generator=g) * (0.78 * (9 * Cin) ** -0.5)).to(bf)
        bias = torch.full((4,), float("nan"))
        bias[:3] = torch.randn(3, generator=g) * 0.05
        n = B * H * W * 3
        for offset in (0, 1):                            # dword stores where W % 4 == 0; one byte past a dword: byte stores
            buf = T8.guarded_out(n, T8.GUARD_BYTE, offset)
            ops.conv3x3_rgb8(x, wt.cuda(), bias.cuda(), out=buf[T8.GUARD + offset:T8.GUARD + offset + n].view(B, H, W, 3))
            yield _line("conv3x3_rgb8_kernel", f"{p.id}-offset{offset}", buf)
    for p in TE.CONV_CASES:
        B, H, W, N, fmt, rotate = p.values
        g = _gen("rgb_in " + p.id)
        img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
        _keep, view, _vals = TE.conv_operand(img, fmt)
        wt = torch.full((N, 32), float("nan"), dtype=bf)
        wt[:, :27] = (torch.randn(N, 27, generator=g) * 27 ** -0.5).to(bf)
        buf, out = R.guarded(B * H * W, N, N, bf, "cuda")
        ops.conv3x3_rgb_in(view, wt.cuda(), (torch.randn(N, generator=g) * 0.3).cuda(), rotate=bool(rotate), out=out.view(B, H, W, N))
        yield _line("conv3x3_rgb_in_kernel", p.id, buf)


def compare(path_a, path_b):
    a, b = ([ln.split() for ln in open(p) if ln.strip()] for p in (path_a, path_b))
    keys_a, keys_b = [tuple(r[:2]) for r in a], [tuple(r[:2]) for r in b]
    diff = sum(ra[2:] != rb[2:] for ra, rb in zip(a, b)) if keys_a == keys_b else -1
    print(f"{'kernel':<26s} {'case':<42s} {os.path.basename(path_a):<18s} {os.path.basename(path_b):<18s} bytes")
    for ra, rb in zip(a, b):
        print(f"{ra[0]:<26s} {ra[1]:<42s} {ra[2][:16]:<18s} {rb[2][:16]:<18s} {ra[3]:>9s} {'' if ra == rb else '  <-- DIFFERS'}")
    if diff < 0:
        print("verdict: the two files do not list the same kernels and cases")
    else:
        print(f"verdict: {len(a)} outputs of {len(set(k[0] for k in keys_a))} kernels, {diff} differ (the first 16 hex digits of each SHA-256 are shown; all 64 are compared)")
    return 1 if diff else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    for line in digest_lines():
        print(line, flush=True)
