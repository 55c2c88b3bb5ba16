#!/usr/bin/env python3
"""Per-kernel register / scratch / occupancy table of lib/libdpe_mvs.so's translation units (hipcc
-Rpass-analysis=kernel-resource-usage): the units and flags of dpe-mvs_amd/Makefile's table, compiled
once more into a scratch folder.  Usage: python tools/ru.py [extra hipcc flags...]"""
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = __file__.rsplit("/tools/", 1)[0]
objdir = tempfile.mkdtemp(prefix="dpe_ru_")
try:
    out = subprocess.run(["make", "-C", ROOT + "/dpe-mvs_amd", "-j16", "-Otarget", "OBJDIR=" + objdir, "objects",
                          "EXTRA_FLAGS=" + " ".join(["-Rpass-analysis=kernel-resource-usage"] + sys.argv[1:])],
                         capture_output=True, text=True)
finally:
    shutil.rmtree(objdir, ignore_errors=True)
if out.returncode:
    sys.exit(out.stdout + out.stderr)
rows, cur = [], None
for line in (out.stdout + out.stderr).splitlines():
    m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
    if not m:
        continue
    k, v = ("Spill" if m.group(1) == "VGPRs Spill" else m.group(1).split()[0]), m.group(2)
    if k == "Function":
        cur = {"name": subprocess.run(["c++filt", v], capture_output=True, text=True).stdout.strip()}
        rows.append(cur)
    elif cur is not None:
        cur[k] = v
for r in rows:
    n = re.sub(r"\(.*", "", r["name"]).replace("dpe::", "")
    print(f"{n:40s} vgpr {r.get('VGPRs','?'):>4} scratch {r.get('ScratchSize','?'):>5} spill {r.get('Spill','?'):>4} occ {r.get('Occupancy','?'):>2} lds {r.get('LDS','?')}")
