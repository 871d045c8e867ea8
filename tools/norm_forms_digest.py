"""SHA-256 of every output of every case of tests/norm_form_cases.py, launched exactly as tests/test_norm_forms_gpu.py launches it (its _Run: the
C entries through ctypes, NaN-padded operands, guarded outputs).  One line per case and output: "<case> <output> <sha256> <bytes>"; the guard rows
behind an output are part of what is hashed.  The inputs are seeded by the case names, so two trees that compute the same bytes print the same text:
    python tools/norm_forms_digest.py > a.txt      (here)
    python tools/norm_forms_digest.py > b.txt      (in a tree of the commit to compare with, built on its own)
    python tools/norm_forms_digest.py --compare a.txt b.txt
--compare prints both columns side by side and the verdict; it needs no GPU.  Nothing is compared with a reference here: that is the test's job."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def digest_lines():
    import torch
    import norm_form_cases as NC
    from test_norm_forms_gpu import _Run
    dev = torch.device("cuda:0")
    for c in NC.ALL_CASES:
        for name, out in sorted(_Run(c, dev).launch().items()):
            raw = out.contiguous().view(torch.uint8).cpu().numpy().tobytes()
            yield f"{c['name']} {name} {hashlib.sha256(raw).hexdigest()} {len(raw)}"


def compare(path_a, path_b):
    a, b = ([ln.split() for ln in open(p) if ln.strip()] for p in (path_a, path_b))
    keys_a, keys_b = [tuple(r[:2]) for r in a], [tuple(r[:2]) for r in b]
    diff = sum(ra[2:] != rb[2:] for ra, rb in zip(a, b)) if keys_a == keys_b else -1
    print(f"{'case':<34s} {'output':<6s} {os.path.basename(path_a):<18s} {os.path.basename(path_b):<18s} bytes")
    for ra, rb in zip(a, b):
        print(f"{ra[0]:<34s} {ra[1]:<6s} {ra[2][:16]:<18s} {rb[2][:16]:<18s} {ra[3]:>8s} {'' if ra == rb else '  <-- DIFFERS'}")
    if diff < 0:
        print("verdict: the two files do not list the same cases and outputs")
    else:
        print(f"verdict: {len(a)} outputs of {len(set(k[0] for k in keys_a))} cases, {diff} differ (the first 16 hex digits of each SHA-256 are shown; all 64 are compared)")
    return 1 if diff else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    for line in digest_lines():
        print(line, flush=True)
