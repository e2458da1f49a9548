"""One sha256 per kernel source of a tree: the device assembly the library's own flags produce for it.

Each .hip file of build.SOURCES is compiled to gfx950 assembly (build.HIPCC_FLAGS without -shared, build.EXTRA_FLAGS[src],
-x hip --cuda-device-only -S), the lines that carry the toolchain's per-source `__hip_cuid_<hash>` symbol are dropped, and
the rest is hashed.  Two trees whose lists agree ship the same device code: what a refactor of the kernel headers has to
show before anything is measured.  The tool hashes only; it does not look at the instructions.
    python tools/kernel_text.py [--tree DIR] [--jobs N] [--keep DIR] [source.hip ...]
--tree: the checkout to compile (default: this one).  --keep: leave the filtered texts there (for a diff of two trees)."""
import argparse, hashlib, importlib.util, os, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
ap.add_argument("--keep", default=None)
ap.add_argument("sources", nargs="*")
args = ap.parse_args()

spec = importlib.util.spec_from_file_location("bn_build", os.path.join(args.tree, "benchnav_amd", "build.py"))
b = importlib.util.module_from_spec(spec)
spec.loader.exec_module(b)
sources = args.sources or [s for s in b.SOURCES if s.endswith(".hip")]
flags = [f for f in b.HIPCC_FLAGS if f != "-shared"]


def kernel_text(src, tmp):
    out = os.path.join(tmp, os.path.splitext(src)[0] + ".s")
    # relative source name, run inside csrc/: no path of the checkout reaches the text
    subprocess.check_call([b.hipcc(), *flags, *b.EXTRA_FLAGS.get(src, []), "-x", "hip", "--cuda-device-only", "-S", src, "-o", out],
                          cwd=b.CSRC)
    with open(out, "rb") as f:
        text = b"".join(line for line in f if b"__hip_cuid_" not in line)
    if args.keep:
        os.makedirs(args.keep, exist_ok=True)
        with open(os.path.join(args.keep, os.path.basename(out)), "wb") as f:
            f.write(text)
    os.remove(out)
    return hashlib.sha256(text).hexdigest()


with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(args.jobs) as pool:
    for src, digest in zip(sources, pool.map(lambda s: kernel_text(s, tmp), sources)):
        print(digest, src)
        sys.stdout.flush()
