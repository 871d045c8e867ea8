"""SHA-256 of every output of the attention launcher (csrc/attention.hip) over the cases its tests run, imported from those files: ATTN_CASES of
tests/kernel_form_cases.py (run by tests/test_kernel_forms_gpu.py's run_attn_case, whose guarded O buffer is hashed), the XCD-map and key-chunk cases of
tests/test_attention_bits_gpu.py, RAGGED_MOVES of tests/test_ops_gpu.py and GROUPED_ATTN_SPECS of tests/test_grouped_gpu.py.  One line per output:
"<kernel> <case> <sha256> <bytes>"; where an output lies in a guarded buffer the guards are part of what is hashed.  The inputs are seeded by the cases, so two
trees that compute the same bytes print the same text:
    python tools/attn_digest.py > a.txt      (here)
    python tools/attn_digest.py > b.txt      (in a tree of the commit to compare with, built on its own; or with MXDENOISE_LIB naming its library)
    python tools/attn_digest.py --compare a.txt b.txt
--compare prints both columns side by side and the verdict; it needs no GPU.  Nothing is compared with a reference here: that is the tests' job."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _line(kernel, name, buf):
    import torch
    raw = buf.contiguous().view(torch.uint8).cpu().numpy().tobytes()
    return f"{kernel.replace(' ', '')} {name} {hashlib.sha256(raw).hexdigest()} {len(raw)}"


def digest_lines():
    import torch
    import kernel_form_cases as KC
    import kernel_ref as R
    import test_attention_bits_gpu as TB
    import test_grouped_gpu as TG
    import test_kernel_forms_gpu as TK
    import test_ops_gpu as TO
    from sduss_amd import lib, ops
    dev = torch.device("cuda:0")
    bf = torch.bfloat16
    # the form matrix: run_attn_case allocates one guarded buffer, O
    made = []
    guarded = R.guarded
    R.guarded = lambda *a, **kw: made.append(guarded(*a, **kw)) or made[-1]
    try:
        for c in KC.ATTN_CASES:
            del made[:]
            TK.run_attn_case(c, dev)
            yield _line(c["target"], c["name"], made[0][0])
    finally:
        R.guarded = guarded
    for kernel, ((lq, lk), (clq, clk)) in TB.CASES.items():
        whole, parts = TB.xcd_case(kernel, lq, lk, dev)
        yield _line(kernel, f"xcd-whole-lq{lq}-lk{lk}", whole)
        yield _line(kernel, f"xcd-slices-lq{lq}-lk{lk}", parts)
        chunked, plain = TB.chunk_case(kernel, clq, clk, dev)
        yield _line(kernel, f"chunks2-lq{clq}-lk{clk}", chunked)
        yield _line(kernel, f"contiguous-lq{clq}-lk{clk}", plain)
    for lq, lk, kernel, spikes in TO.RAGGED_MOVES:
        q, k, v = TO.ragged_moves_inputs(lq, lk, spikes)
        qs = TO._rt(q * ops.ATTN_QSCALE)
        o = ops.attention(qs.reshape(-1, 64).to(bf).cuda(), k.reshape(-1, 64).to(bf).cuda(), ops.pack_vt(v, pad=float("nan")).to(bf).cuda(), 1, lq, lk, prescaled=True)
        yield _line(kernel, f"ragged-moves-lq{lq}-lk{lk}", o)
    heads = 5
    c = heads * 64
    for n, (spec, lk_fixed) in enumerate(TG.GROUPED_ATTN_SPECS):
        g = torch.Generator().manual_seed(sum(b * L for b, L in spec) + (lk_fixed or 0))
        probs = (lib.AttnProblem * len(spec))()
        keep = []
        for i, (b, lq) in enumerate(spec):
            lk = lk_fixed or lq
            q, k, v = (torch.randn(b, l, c, generator=g).to(bf) for l in (lq, lk, lk))
            qg, kg, vg = (q.float() * ops.ATTN_QSCALE).to(bf).reshape(-1, c).cuda(), k.reshape(-1, c).cuda(), ops.pack_vt(v).cuda()
            obuf, o = R.guarded(b * lq, c, c, bf, dev)
            keep.append((qg, kg, vg, obuf))
            probs[i].q, probs[i].k, probs[i].vt, probs[i].o = qg.data_ptr(), kg.data_ptr(), vg.data_ptr(), o.data_ptr()
            probs[i].vt_batch_stride, probs[i].B, probs[i].Lq, probs[i].Lk, probs[i].ldvt = c * vg.shape[-1], b, lq, lk, vg.shape[-1]
        lib.check(lib.load().mx_attention_prescaled_grouped(lib.current_stream(), probs, len(spec), c, c, c, heads), "grouped attention")
        torch.cuda.synchronize()
        for i, (b, lq) in enumerate(spec):
            yield _line("grouped", f"spec{n}-problem{i}-b{b}-lq{lq}-lk{lk_fixed or lq}", keep[i][3])


def compare(path_a, path_b):
    a, b = ([ln.split() for ln in open(p) if ln.strip()] for p in (path_a, path_b))
    keys_a, keys_b = [tuple(r[:2]) for r in a], [tuple(r[:2]) for r in b]
    diff = sum(ra[2:] != rb[2:] for ra, rb in zip(a, b)) if keys_a == keys_b else -1
    print(f"{'kernel':<30s} {'case':<42s} {os.path.basename(path_a):<18s} {os.path.basename(path_b):<18s} bytes")
    for ra, rb in zip(a, b):
        print(f"{ra[0]:<30s} {ra[1]:<42s} {ra[2][:16]:<18s} {rb[2][:16]:<18s} {ra[3]:>9s} {'' if ra == rb else '  <-- DIFFERS'}")
    if diff < 0:
        print("verdict: the two files do not list the same kernels and cases")
    else:
        print(f"verdict: {len(a)} outputs, {diff} differ (the first 16 hex digits of each SHA-256 are shown; all 64 are compared)")
    return 1 if diff else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    for line in digest_lines():
        print(line, flush=True)
