"""In-job A/B of a kernel change: builds extra libraries from the in-tree sources with the files of an override directory put on
top (e.g. an older revision of one .hip), then runs a probe script alternately against all of them in the same gpurun job
(box-to-box variance is +-4%, so only same-job comparisons are meaningful).

    python tools/ab.py <override_dir>[,<override_dir>...] <probe.py> [rounds]

An override "dir" of the form  NAME=VALUE  instead builds the in-tree sources with -DNAME=VALUE (diagnostic switches that only
exist in scratch copies).  The probe gets the library to use in argv[1] ("" = in-tree) and a tag in argv[2]."""
import os, shutil, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ovrs, probe = sys.argv[1].split(","), sys.argv[2]
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 2
libs = [("in-tree", "")]
tmps = []
for o in ovrs:
    tmp = tempfile.mkdtemp(prefix="conan_ab_"); tmps.append(tmp)
    os.makedirs(os.path.join(tmp, "include")); shutil.copy(os.path.join(ROOT, "include", "conan_fgw_hip.h"), os.path.join(tmp, "include"))
    src = os.path.join(tmp, "pkg", "csrc"); shutil.copytree(os.path.join(ROOT, "conan-fgw_amd", "csrc"), src, ignore=shutil.ignore_patterns("*.o", "*.d"))
    extra = []
    if "=" in o and not os.path.isdir(o):
        extra = ["CXXFLAGS=-O3 -fPIC -std=c++17 --offload-arch=gfx950 -Wno-unused-function -D" + o]
    else:
        for f in os.listdir(o):
            shutil.copy(os.path.join(o, f), os.path.join(src, f))
    subprocess.check_call(["make", "-C", src, "-s", "-j16"] + extra, stderr=subprocess.DEVNULL)
    libs.append((os.path.basename(o.rstrip("/")), os.path.join(tmp, "pkg", "libconan_fgw_hip.so")))
w = max(len(t) for t, _ in libs)
for rnd in range(rounds):
    for tag, so in libs:
        subprocess.check_call([sys.executable, probe, so, tag.ljust(w)])
for t in tmps:
    shutil.rmtree(t, ignore_errors=True)
