"""Per-kernel register / LDS / code-size table of the product library, from the compiler's own resource report (no GPU needed):

    python tools/kernel_resources.py > profiles/r06_kernel_resources.txt
    python tools/kernel_resources.py kernels_attn_wide.hip > profiles/attn_wide_resources.txt      # some translation units only
    python tools/kernel_resources.py --digest [--csrc DIR] > new.txt       # one digest of the instruction text per kernel, sorted by name: diff two trees

Columns: VGPRs + AGPRs one wave allocates (gfx950: 512 per SIMD lane, shared by every resident wave of the SIMD), waves per SIMD one workgroup
brings (threads / 256), the share of a SIMD's register file ONE workgroup takes, static LDS, code bytes.  A CU hosts two workgroups only if
their register shares AND their LDS both fit -- profiles/r06_notes.md section 2 reads the step's collisions off this table.

--digest: did a change of the sources change a kernel's machine code?  Per kernel the text between its label and its last s_endpgm, comments
stripped and the local block labels (.LBB<n>_<m>) renumbered in order of appearance, as SHA-1 + instruction count + the resource columns; the
translation unit is not part of a row, so a kernel that moved to another file compares equal.  --csrc DIR reads another source tree (the
directory tools/build_base.py unpacks a revision into)."""
import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'vslnet_amd', 'csrc')
sys.path.insert(0, ROOT)
from vslnet_amd.build import FLAGS, FILE_FLAGS, _hipcc      # noqa: E402

THREADS = {'k_convblock_fwd2': 512, 'k_convblock_fwd': 512, 'k_convblock_bwd': 512, 'k_attn_block_fwd<1': 1024, 'k_attn_block_fwd<2': 512, 'k_attn_bwd_fused': 1024,
           'k_attn_bwd_long': 1024, 'k_wgrad4': 512, 'k_wgrad3': 256, 'k_vproj_fwd3': 512, 'k_embed_fwd': 512, 'k_embed_bwd': 512, 'k_query_fwd': 256, 'k_query_bwd': 256}


def demangle(names):
    r = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True)
    return r.stdout.split('\n')


def code_digest(txt, name):
    """(SHA-1, instruction count) of kernel `name`'s instruction text in the assembly listing `txt`"""
    body = txt[txt.index('\n' + name + ':') + len(name) + 2:txt.index('.Lfunc_end', txt.index('\n' + name + ':'))]
    body = body[:body.rindex('s_endpgm') + len('s_endpgm')]
    labels, lines, n = {}, [], 0
    for line in body.split('\n'):
        line = ' '.join(line.split(';')[0].split())
        if not line:
            continue
        line = re.sub(r'\.LBB\d+_\d+', lambda m: labels.setdefault(m.group(0), '.L%d' % len(labels)), line)
        n += not line.endswith(':') and not line.startswith('.')
        lines.append(line)
    return hashlib.sha1('\n'.join(lines).encode()).hexdigest()[:16], n


def assembly(csrc, src):
    cmd = [_hipcc()] + [f for f in FLAGS if f != '-fPIC'] + FILE_FLAGS.get(src, []) + ['--cuda-device-only', '-S', os.path.join(csrc, src), '-o', '-']
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def main():
    argv, csrc = sys.argv[1:], CSRC
    digest = '--digest' in argv
    if '--csrc' in argv:
        csrc = argv[argv.index('--csrc') + 1]
        argv.remove(csrc)
    argv = [a for a in argv if not a.startswith('--')]
    units = [s for s in argv or sorted(f for f in os.listdir(csrc) if f.endswith('.hip')) if '__global__' in open(os.path.join(csrc, s)).read()]   # not the host-only units
    with ThreadPoolExecutor(16) as ex:
        listings = list(ex.map(lambda s: assembly(csrc, s), units))
    rows = []
    for src, txt in zip(units, listings):
        for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', txt, re.S):
            name, body = m.group(1), m.group(2)
            lds = int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', body).group(1))
            info = txt[txt.find('.size\t' + name):]
            code = int(re.search(r'; codeLenInByte = (\d+)', info).group(1))
            v = int(re.search(r'; NumVgprs: (\d+)', info).group(1))
            a = int(re.search(r'; NumAgprs: (\d+)', info).group(1))
            scr = int(re.search(r'; ScratchSize: (\d+)', info).group(1))
            rows.append((src, name, v, a, lds, code, scr) + (code_digest(txt, name) if digest else ()))
    dn = demangle([r[1] for r in rows])
    if digest:
        print('# instruction text per kernel (hipcc --offload-arch=gfx950 -S, the build\'s flags): SHA-1 of the text between the label and s_endpgm, comments')
        print('# stripped, block labels renumbered; tools/kernel_resources.py --digest')
        print('%-16s %6s %5s %5s %8s %7s  %s' % ('sha1', 'instr', 'VGPR', 'AGPR', 'LDS', 'scratch', 'kernel'))
        for (src, name, v, a, lds, code, scr, dg, n), d in sorted(zip(rows, dn), key=lambda x: x[1]):
            print('%-16s %6d %5d %5d %8d %7d  %s' % (dg, n, v, a, lds, scr, re.sub(r'^void ', '', d).replace('vsl::', '')))
        return
    print('# compiler resource report of vslnet_amd/csrc (hipcc --offload-arch=gfx950, the build\'s flags); tools/kernel_resources.py')
    print('# regs = VGPRs + AGPRs per lane of one wave (allocated in blocks of 8; 512 per SIMD lane); w/SIMD = waves one workgroup puts on a SIMD;')
    print('# share = w/SIMD x ceil8(regs) / 512 of the register file ONE workgroup takes; LDS = static bytes (dynamic LDS: see the launchers)')
    print('%-92s %5s %5s %6s %6s %8s %7s %7s' % ('kernel', 'VGPR', 'AGPR', 'w/SIMD', 'share', 'LDS', 'code B', 'scratch'))
    for (src, name, v, a, lds, code, scr), d in zip(rows, dn):
        short = re.sub(r'\(.*', '', d).replace('void vsl::', '').replace('vsl::', '')
        thr = 256
        for k, t in THREADS.items():
            if short.startswith(k):
                thr = t
        wps = thr // 256
        regs = (v + a + 7) // 8 * 8
        print('%-92s %5d %5d %6d %5.0f%% %8d %7d %7d' % (short[:92], v, a, wps, 100.0 * wps * regs / 512, lds, code, scr))


if __name__ == '__main__':
    main()
