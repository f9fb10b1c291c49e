"""Builds lib3dvnet_hip.so in-tree with hipcc for gfx950 (no cmake, no JIT cache).

    python 3dvnet_amd/build.py [--force] [--verbose]

The .so is git-ignored but travels to the GPU box with the repo snapshot.
"""
import glob
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'lib3dvnet_hip.so')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wall', '-Wno-unused-function',
         '-I', os.path.join(ROOT, 'include'), '-I', CSRC] + os.environ.get('V3D_EXTRA_FLAGS', '').split()


def sources():
    return sorted(glob.glob(os.path.join(CSRC, '*.hip')))


def _flags_tag():
    """Objects are keyed by the compiler flags: a build with V3D_EXTRA_FLAGS (the developer scripts' instrumented /
    ablated variants) lands in its own object directory and can never be mistaken for the default build."""
    return hashlib.sha256(' '.join([HIPCC] + FLAGS).encode()).hexdigest()[:12]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False, strict=False):
    """Compile every csrc/*.hip to an object (in parallel) and link the shared library."""
    headers = glob.glob(os.path.join(CSRC, '*.h')) + glob.glob(os.path.join(ROOT, 'include', '*.h'))
    tag = _flags_tag()
    objdir = os.path.join(HERE, 'build', tag)
    os.makedirs(objdir, exist_ok=True)
    stamp = os.path.join(HERE, 'build', 'linked_flags')     # which flag set the in-tree .so was linked from
    linked = open(stamp).read().strip() if os.path.exists(stamp) else None
    procs, objs = [], []
    for src in sources():
        obj = os.path.join(objdir, os.path.basename(src)[:-4] + '.o')
        objs.append(obj)
        if force or _stale(obj, [src] + headers):
            cmd = [HIPCC] + FLAGS + ['-c', src, '-o', obj]
            if verbose:
                print(' '.join(cmd))
            procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            sys.stderr.write(out.decode())
            raise RuntimeError('hipcc failed on %s' % src)
        if verbose and out:
            print(out.decode())
    # ISA guard of the fused decoder (3dvnet_amd/isa_check.py: no scratch; LDS read signature pinned per compiler version) on the
    # default build; developer flag sets are not checked.  `strict` (the entry-point build): the guard must be able to run.
    if not os.environ.get('V3D_EXTRA_FLAGS', '').strip() and not os.environ.get('V3D_SKIP_LDS_CHECK'):
        sys.path.insert(0, HERE)
        try:
            import isa_check
            isa_check.check(os.path.join(objdir, 'decoder.o'), strict=strict)
            # the fused backbone kernels: every 16-byte LDS read must be the operand of a matrix instruction
            isa_check.check_wide_lds(os.path.join(objdir, 'irb.o'), 'irb_kernel', strict=strict)
            isa_check.check_wide_lds(os.path.join(objdir, 'fpn.o'), 'fpn_level_kernel', strict=strict)
            # stage 3: the layer-4 softmax epilogue reads its logits 8 / 4 bytes at a time beside the layer-1 matrix wave
            isa_check.check_wide_lds(os.path.join(objdir, 'propz.o'), 'propz_kernel', strict=strict)
            # depth fusion: the per-pixel chain of fuse_depths_kernel stays in registers
            isa_check.check_no_scratch(os.path.join(objdir, 'fusion.o'), 'fuse_depths_kernel', strict=strict)
            # TSDF integration: the five running values of a voxel stay in registers across the view loop
            isa_check.check_no_scratch(os.path.join(objdir, 'tsdf.o'), 'tsdf_integrate_kernel', strict=strict)
            # TSDF resampling: the coordinate, the eight tap indices and weights of an output voxel stay in registers
            isa_check.check_no_scratch(os.path.join(objdir, 'tsdf_resample.o'), 'tsdf_resample_kernel', strict=strict)
            isa_check.check_no_scratch(os.path.join(objdir, 'tsdf_resample.o'), 'volume_resample_nearest_kernel', strict=strict)
            # nearest neighbour: the per-query search state of nn_query_kernel stays in registers
            isa_check.check_no_scratch(os.path.join(objdir, 'cloudmetrics.o'), 'nn_query_kernel', strict=strict)
            # mesh extraction: the status bytes of a cell, its table row and the vertex state stay in registers
            isa_check.check_no_scratch(os.path.join(objdir, 'mesh.o'), 'mc_[a-z_]*_kernel', strict=strict)
            # mesh rendering: the triangle's nine coordinates, ten plane coefficients and box stay in registers across the views
            isa_check.check_no_scratch(os.path.join(objdir, 'meshrender.o'), 'mesh_render_kernel', strict=strict)
            # plane-sweep warp: the window kernel walks the depth axis at the register limit of 4 waves per SIMD; what it keeps
            # across the walk must stay in registers
            isa_check.check_no_scratch(os.path.join(objdir, 'psv_window.o'), 'psv_variance_window_kernel', strict=strict)
            # its backward: the 16 plane means, the 16 scaled gradients and the four tap sums of a lane stay in registers
            isa_check.check_no_scratch(os.path.join(objdir, 'psv_backward.o'), 'psv_variance_backward_kernel', strict=strict)
            # the back-projected variance's backward: the same state per hypothesis segment; the depth kernel's chains
            isa_check.check_no_scratch(os.path.join(objdir, 'backproject_backward.o'), 'backproject_[a-z]*_backward_kernel',
                                       strict=strict)
            # the sparse interpolation's backward: the 8 slots, weights and gradient rows of a lane in flight stay in registers
            isa_check.check_no_scratch(os.path.join(objdir, 'sparse_interp.o'), 'interp_backward_[a-z]*_kernel', strict=strict)
            # the sparse convolution's weight gradient: up to 4 x 4 accumulator blocks (64 registers) and the 8 staged rows of a lane
            isa_check.check_no_scratch(os.path.join(objdir, 'gemm_wgrad.o'), 'sparse_conv_wgrad_[a-z_]*kernel', strict=strict)
            # confidence: the running maximum, the denominator and the two plane indices of a pixel stay in registers
            isa_check.check_no_scratch(os.path.join(objdir, 'confidence.o'), 'soft_argmin_prob_kernel', strict=strict)
            isa_check.check_no_scratch(os.path.join(objdir, 'confidence.o'), 'prob_gather_kernel', strict=strict)
            # 2D depth metrics: the five double sums and five counters of a lane stay in registers across its pixels
            isa_check.check_no_scratch(os.path.join(objdir, 'depthmetrics.o'), 'depth_metrics_[a-z]*_kernel', strict=strict)
            # depth supervision: the same, with the loss's sum and counter beside them
            isa_check.check_no_scratch(os.path.join(objdir, 'supervision.o'), 'depth_supervision_[a-z]*_kernel', strict=strict)
            # order statistics: the keys of a tile's points and the back-projection stay in registers in every counting pass
            isa_check.check_no_scratch(os.path.join(objdir, 'order_stats.o'), 'order_stats_[a-z]*_kernel', strict=strict)
            # scene batches from frames: the twelve blends of a thread and its table entries stay in registers
            isa_check.check_no_scratch(os.path.join(objdir, 'frames.o'), 'frames_to_images_kernel', strict=strict)
            isa_check.check_no_scratch(os.path.join(objdir, 'frames.o'), 'frames_to_depths_kernel', strict=strict)
            # scene preparation: the four sample positions and the twelve bytes of a thread stay in registers
            isa_check.check_no_scratch(os.path.join(objdir, 'prepare.o'), 'register_colour_kernel', strict=strict)
            isa_check.check_no_scratch(os.path.join(objdir, 'prepare.o'), 'lut_u16_kernel', strict=strict)
        finally:
            sys.path.pop(0)
    if force or procs or linked != tag or _stale(LIB, objs):
        cmd = [HIPCC, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', LIB] + objs
        if verbose:
            print(' '.join(cmd))
        subprocess.check_call(cmd)
        with open(stamp, 'w') as f:
            f.write(tag + '\n')
    return LIB


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose='--verbose' in sys.argv))
