"""Build the geomx_amd native extension (_geops) for gfx950.

    PYTORCH_ROCM_ARCH=gfx950 python setup.py build_ext --inplace

The extension is built IN-TREE (geomx_amd/_geops.*.so) so it travels to
GPU machines with the source snapshot.
"""

import os
import subprocess

from setuptools import setup

os.environ.setdefault("PYTORCH_ROCM_ARCH", "gfx950")

from torch.utils.cpp_extension import (ROCM_HOME, BuildExtension,  # noqa: E402
                                       CppExtension, CUDAExtension)

here = os.path.dirname(os.path.abspath(__file__))

ext = CUDAExtension(
    name="geomx_amd._geops",
    sources=[
        "geomx_amd/csrc/geops.cpp",
        "geomx_amd/csrc/kernels.hip",
        "geomx_amd/csrc/conv.hip",
        "geomx_amd/csrc/convwrw2.hip",
        "geomx_amd/csrc/fc.hip",
        "geomx_amd/csrc/finalize.hip",
        "geomx_amd/csrc/rowsparse.hip",
    ],
    extra_compile_args={
        "cxx": ["-O3", "-std=c++17"],
        "nvcc": ["-O3", "-std=c++17", "--offload-arch=gfx950"],
    },
)

# Kernel files built WITHOUT packed fp32 instructions (v_pk_add/mul/fma_f32):
# their sums are specified one rounded addition at a time and are compiled
# to scalar fp32 VALU ops only. dgtencode.hip is kept to scalar fp32 ops in
# the same way; there the switch changes no result, only registers (204
# VGPRs with packed fp32 on against 156 at chunk 8192, docs/kernels.md).
# wiresparse.hip folds the Bi-Sparse lists in the same stated order.
# conv1c.hip (the CI = 1 conv stage) sums its four waves' slabs in a
# stated order and is built the same way. bscselect.hip forms its keys with
# one rounded multiply and two rounded additions (bsc_mom.h) and is too.
# conv1x32.hip (the conv1 stage from the fp32 image) is too: its kernel is
# the fp32 instantiation of the template in conv5_pool2.h, whose bf16
# instantiation conv.hip keeps building as before; conv1u8.hip is the uint8
# instantiation of the same template, built like its fp32 sibling. lars.hip (layer-wise LARS)
# specifies its sums of squares one rounded operation at a time and is too.
# wirefp8.hip (the FP8 wire tier) adds the residual, subtracts the decoded
# value and folds the parties one rounded operation at a time and is too.
# The extension's flag list is one for all of its sources, so these are
# compiled here, with the same flags plus the feature switch, and linked
# into _geops as objects. They include no torch header.
NO_PK_F32_SOURCES = ["geomx_amd/csrc/wirereduce.hip",
                     "geomx_amd/csrc/wiresparse.hip",
                     "geomx_amd/csrc/dgtencode.hip",
                     "geomx_amd/csrc/conv1c.hip",
                     "geomx_amd/csrc/bscselect.hip",
                     "geomx_amd/csrc/conv1x32.hip",
                     "geomx_amd/csrc/conv1u8.hip",
                     "geomx_amd/csrc/lars.hip",
                     "geomx_amd/csrc/wirefp8.hip"]
NO_PK_F32_DEPENDS = ["geomx_amd/csrc/wire_codec.h",
                     "geomx_amd/csrc/bsc_mom.h",
                     "geomx_amd/csrc/conv5_common.h",
                     "geomx_amd/csrc/conv5_pool2.h",
                     "geomx_amd/csrc/geops_grid.h",
                     "geomx_amd/csrc/optim_rules.h"]
NO_PK_F32_FLAGS = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
ext.depends += NO_PK_F32_SOURCES + NO_PK_F32_DEPENDS


class GeoBuildExtension(BuildExtension):
    def build_extension(self, ext_):
        if ext_ is ext:
            for src in NO_PK_F32_SOURCES:
                obj = os.path.join(self.build_temp,
                                   os.path.splitext(src)[0] + ".o")
                os.makedirs(os.path.dirname(obj), exist_ok=True)
                deps = [os.path.join(here, f)
                        for f in [src] + NO_PK_F32_DEPENDS]
                if not os.path.exists(obj) or any(
                        os.path.getmtime(d) > os.path.getmtime(obj)
                        for d in deps):
                    subprocess.check_call(
                        [os.path.join(ROCM_HOME, "bin", "hipcc"), "-O3",
                         "-std=c++17", "--offload-arch=gfx950", "-fPIC"]
                        + NO_PK_F32_FLAGS
                        + ["-c", os.path.join(here, src), "-o", obj])
                if obj not in ext_.extra_objects:
                    ext_.extra_objects.append(obj)
        super().build_extension(ext_)


# host-side IO runtime (record-file reader) — plain C++, no HIP
io_ext = CppExtension(
    name="geomx_amd._geoio",
    sources=["geomx_amd/csrc/recordio.cpp"],
    extra_compile_args=["-O3", "-std=c++17"],
)

setup(
    name="geomx_amd",
    version="0.1.0",
    packages=["geomx_amd", "geomx_amd.kvstore", "geomx_amd.ops",
              "geomx_amd.parallel", "geomx_amd.models", "geomx_amd.utils"],
    ext_modules=[ext, io_ext],
    cmdclass={"build_ext": GeoBuildExtension},
)
