"""Build vslnet_amd/lib/libvslnet_hip_<name>.so (default name: base) from the sources of a git revision (default HEAD), for same-box A/B runs:
    python tools/build_base.py <rev> [name]
    VSLNET_HIP_LIB=vslnet_amd/lib/libvslnet_hip_base.so python bench.py ...   vs   python bench.py ..."""
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
rev = sys.argv[1] if len(sys.argv) > 1 else 'HEAD'
name = sys.argv[2] if len(sys.argv) > 2 else 'base'          # -> vslnet_amd/lib/libvslnet_hip_<name>.so
tmp = '/tmp/vsl_base_src'
if os.path.isdir(tmp):
    shutil.rmtree(tmp)
# the revision's own file list: it may have other translation units than this tree
files = subprocess.check_output(['git', 'ls-tree', '-r', '--name-only', rev, 'vslnet_amd/csrc', 'include'], cwd=ROOT, text=True).split()
for f in files:
    os.makedirs(os.path.dirname(os.path.join(tmp, f)), exist_ok=True)
    open(os.path.join(tmp, f), 'wb').write(subprocess.check_output(['git', 'show', '%s:%s' % (rev, f)], cwd=ROOT))
from vslnet_amd import build  # noqa: E402
print(build.build(csrc=os.path.join(tmp, 'vslnet_amd/csrc'), out=os.path.join(ROOT, 'vslnet_amd/lib/libvslnet_hip_%s.so' % name)))
