"""Per-kernel fingerprints of the device code in object files:  python tools/kernel_fingerprint.py a.o [b.o ...]

One sorted line per kernel: the mangled name, a sha256 of its instruction text (llvm-objdump -d, without the address column,
symbol offsets and the padding behind the kernel, so a kernel keeps its hash when it moves inside or between code objects) and the kernel metadata
(llvm-readelf --notes).  Two builds run the same device code when their sets of lines are equal; object files themselves are not
byte-reproducible.  Nothing is searched for: the text is only hashed."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get('XMEM_LLVM_BIN', '/opt/rocm/lib/llvm/bin')
ARCH = 'gfx950'
META = ('vgpr_count', 'agpr_count', 'sgpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size', 'kernarg_segment_size',
        'max_flat_workgroup_size')


def _run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool)] + list(args), check=True, capture_output=True, text=True).stdout


def unbundle(obj, tmp):
    """the gfx950 code object inside a host object (the same two steps as tests/test_host_logic.py)"""
    fat, co = os.path.join(tmp, 'fat.bin'), os.path.join(tmp, 'dev.co')
    _run('llvm-objcopy', '-O', 'binary', '--only-section=.hip_fatbin', obj, fat)
    _run('clang-offload-bundler', '--unbundle', '--type=o', f'--input={fat}', f'--targets=hipv4-amdgcn-amd-amdhsa--{ARCH}', f'--output={co}')
    return co


def fingerprints(obj):
    """{mangled kernel name: (instruction sha256, {metadata key: value})}"""
    with tempfile.TemporaryDirectory() as tmp:
        co = unbundle(obj, tmp)
        asm, notes, syms = _run('llvm-objdump', '-d', co), _run('llvm-readelf', '--notes', co), _run('llvm-readelf', '-sW', co)
    # symbol -> (address, size): a kernel's text ends where its symbol ends; what follows is alignment padding up to the next
    # function, whose length depends on the neighbour and not on the kernel
    extent = {m.group(3): (int(m.group(1), 16), int(m.group(2), 0))
              for m in re.finditer(r'^\s*\d+:\s+([0-9a-f]+)\s+(\S+)\s+FUNC\s+\S+\s+\S+\s+\S+\s+(\S+)$', syms, re.M)}
    meta = {}
    for entry in re.split(r'\n  - (?=\.)', notes):                    # one item of the amdhsa.kernels list per kernel
        name = re.search(r'\.name:\s+(\S+)', entry)
        if name and '.kernarg_segment_size' in entry:
            meta[name.group(1)] = {k: int(re.search(rf'\.{k}:\s+(\d+)', entry).group(1)) for k in META}
    text = {}
    for body in re.split(r'\n(?=[0-9a-f]+ <)', asm):
        head = re.match(r'[0-9a-f]+ <(\S+)>:', body)
        if not head or head.group(1) not in meta:
            continue
        start, size = extent[head.group(1)]
        lines = []
        for line in body.splitlines()[1:]:
            m = re.match(r'\s*(\S.*?)\s*//\s*([0-9A-Fa-f]+):', line)  # instruction // address: encoding <symbol + offset>
            if m and int(m.group(2), 16) < start + size:
                lines.append(m.group(1))
        text[head.group(1)] = hashlib.sha256('\n'.join(lines).encode()).hexdigest()
    assert set(text) == set(meta), f'{obj}: kernels in the metadata and in the disassembly differ'
    return {n: (text[n], meta[n]) for n in meta}


def main(objs):
    rows = {}
    for obj in objs:
        for name, (sha, meta) in fingerprints(obj).items():
            assert name not in rows, f'{name} is defined in two objects'
            rows[name] = f'{name} {sha} ' + ' '.join(f'{k}={meta[k]}' for k in META)
    for name in sorted(rows):
        print(rows[name])
    print(f'{len(rows)} kernels', file=sys.stderr)


if __name__ == '__main__':
    main(sys.argv[1:])
