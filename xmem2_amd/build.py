"""Build the gfx950 shared library (plain hipcc, no torch headers - the boundary is a C ABI).

``python -m xmem2_amd.build`` or ``__graft_entry__.build()``.  The library is built IN-TREE
(xmem2_amd/csrc/libxmem_hip.so) so that it travels to the GPU box with the repo snapshot.
"""
import os
import shutil
import subprocess
import sys

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'csrc')
SOURCES = ['conv.hip', 'conv_mfma.hip', 'conv_winograd.hip', 'gemm_stream.hip', 'pointwise_pair.hip', 'elementwise.hip', 'affinity.hip', 'affinity_filter.hip', 'consolidate.hip', 'selector.hip', 'augment.hip', 'metrics.hip', 'click.hip', 'brs.hip', 'edt.hip', 'resize_u8.hip', 'copy_segments.hip', 'rle.hip', 'store_compact.hip', 'components.hip', 'polygons.hip', 'polygons_fill.hip', 'matte.hip', 'temporal.hip', 'png.hip', 'motion.hip', 'confidence.hip']
HEADERS = ['common.hpp', 'host_math.hpp', 'affinity_common.hpp', 'conv_plan.hpp', 'conv_mfma.hpp', 'conv_winograd.hpp', 'gemm_stream.hpp',
           'pointwise_pair.hpp', 'vote_bytes.hpp']
LIB = os.path.join(CSRC, 'libxmem_hip.so')
ARCH = 'gfx950'
EXTRA_FLAGS = {'augment.hip': ['-ffp-contract=off']}      # per-source flags: the augmentation kernel rounds where the host libraries round
# NO PACKED-FP32 VALU INSTRUCTIONS (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32) in any kernel of this library.  Measured on MI355X
# (round 3, tools/probes/victim_decoder_probe.py, hog_probe.py): an elementwise kernel built with them returned wrong values
# in ~1e-4 of its elements (one 32-bit half of a packed result) WHILE a kernel issuing v_mfma_f32_32x32x16_f16 ran on another
# stream - the memory-readout filter and the split-operand GEMMs do exactly that next to the side-stream key encoder.  With
# the subtarget feature turned off the same runs are bit-identical to the solo runs.  (The flag reaches the host compilation
# too, which prints an 'ignoring feature' note - filtered below.)
INCLUDE = os.path.join(os.path.dirname(CSRC), '..', 'include')
PUBLIC_HEADERS = ['xmem_hip.h', 'xmem_hip_masks.h', 'xmem_hip_polygons.h']      # the frozen ABI-5 header and the two that declare what came after it
# headers that came after the list above was pinned, as paths in the include directory this module found at import
LATER_HEADERS = [os.path.join(INCLUDE, f) for f in ('xmem_hip_raster.h',)]
# the fifth header (mattes, trimaps, grow / shrink): the two lists above are pinned to their contents, so it has a list of its own
MATTE_HEADERS = [os.path.join(INCLUDE, f) for f in ('xmem_hip_matte.h',)]
# the sixth header (the temporal majority vote), for the same reason
TEMPORAL_HEADERS = [os.path.join(INCLUDE, f) for f in ('xmem_hip_temporal.h',)]
# the seventh header (PNG files built on the device), for the same reason
PNG_HEADERS = [os.path.join(INCLUDE, f) for f in ('xmem_hip_png.h',)]
# the eighth header (confidence and uncertainty maps), for the same reason
CONFIDENCE_HEADERS = [os.path.join(INCLUDE, f) for f in ('xmem_hip_confidence.h',)]
# the ninth header (luma, block motion, the motion-compensated vote), for the same reason
MOTION_HEADERS = [os.path.join(INCLUDE, f) for f in ('xmem_hip_motion.h',)]
DEVICE_FLAGS = ['-Xclang', '-target-feature', '-Xclang', '-packed-fp32-ops']
_NOISE = "'-packed-fp32-ops' is not a recognized feature for this target (ignoring feature)"


def _hipcc():
    for cand in (os.environ.get('HIPCC'), shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError('hipcc not found: the MI355X kernels cannot be built (no CPU fallback exists)')


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS]
    deps += [os.path.join(INCLUDE, f) for f in PUBLIC_HEADERS] + LATER_HEADERS + MATTE_HEADERS + TEMPORAL_HEADERS + PNG_HEADERS + CONFIDENCE_HEADERS + MOTION_HEADERS
    return any(os.path.getmtime(d) > t for d in deps)


def source_digest():
    """sha256 over the kernel sources + headers: profiles recorded for one build are only quoted against the same build."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(SOURCES + HEADERS):
        with open(os.path.join(CSRC, f), 'rb') as fh:
            h.update(fh.read())
    for f in PUBLIC_HEADERS:
        with open(os.path.join(INCLUDE, f), 'rb') as fh:
            h.update(fh.read())
    for path in LATER_HEADERS + MATTE_HEADERS + TEMPORAL_HEADERS + PNG_HEADERS + CONFIDENCE_HEADERS + MOTION_HEADERS:
        with open(path, 'rb') as fh:
            h.update(fh.read())
    h.update(' '.join(DEVICE_FLAGS).encode())
    for src in sorted(EXTRA_FLAGS):
        h.update((src + ':' + ' '.join(EXTRA_FLAGS[src])).encode())
    h.update(os.environ.get('XMEM_HIPCC_FLAGS', '').encode())
    return h.hexdigest()[:16]


def build(force=False, verbose=True):
    if not force and not needs_build():
        return LIB
    hipcc = _hipcc()
    objs = []
    procs = []
    for src in SOURCES:
        obj = os.path.join(CSRC, src.replace('.hip', '.o'))
        objs.append(obj)
        cmd = [hipcc, f'--offload-arch={ARCH}', '-O3', '-std=c++17', '-fPIC'] + DEVICE_FLAGS + EXTRA_FLAGS.get(src, []) + \
              os.environ.get('XMEM_HIPCC_FLAGS', '').split() + ['-x', 'hip', '-c', os.path.join(CSRC, src), '-o', obj]
        if verbose:
            print(' '.join(cmd), flush=True)
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f'hipcc failed on {src}:\n{out}')
        out = '\n'.join(l for l in out.splitlines() if _NOISE not in l and l.strip())
        if verbose and out.strip():
            print(out)
    cmd = [hipcc, f'--offload-arch={ARCH}', '-shared', '-fPIC', '-o', LIB] + objs
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return LIB


if __name__ == '__main__':
    build(force='--force' in sys.argv)
    print('built', LIB)
