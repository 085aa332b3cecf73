"""The inputs of the reference's own known-answer vectors for the convolutions (unittests/math_convlt.cxx), shared by the oracle tests and the GPU tests."""
import numpy as np


# unittests/math_convlt.cxx case 0 passes the FLOAT kernel of CompVMathGauss::kernelDim1(7, 3.5) to the u16 fixed-point entry
# point (:143 builds it with kernelDim1, :66-70 reinterprets it): the 7 "weights" are the first 14 bytes of 7 floats.  They are
# committed here as data (generated with the compiled reference on this toolchain's libm) so the vector is usable anywhere.
CASE0_KERNEL_LITERAL = [16002, 15852, 56670, 15888, 48169, 15907, 36460, 15914, 48169, 15907, 56670, 15888, 16002, 15852]


def case0_input():
    W, H, S = 1285, 720, 1344                                                  # unittests/math_convlt.cxx:21
    j, i = np.mgrid[0:H, 0:W]
    d = np.zeros((H, S), np.uint8)
    d[:, :W] = ((i * j) + 53).astype(np.uint8)                                  # :96
    return d[:, :W]


def convlt_inputs():
    # unittests/math_convlt.cxx:100-165: 1285x720, stride 1344, k = 7
    W, H, S = 1285, 720, 1344
    i = np.arange(W)[None, :]
    j = np.arange(H)[:, None]
    d8 = np.zeros((H, S), np.uint8)
    d8[:, :W] = ((i * j) + 53).astype(np.uint8)                               # :107
    d16 = np.zeros((H, S), np.int16)
    d16[:, :W] = (((i * j) + 53) * np.where(i & 1, -1, 1)).astype(np.int16)    # :129
    k = np.array([(t + 53) * (-1 if t & 1 else 1) for t in range(7)], np.int16)  # :158
    return d8[:, :W], d16[:, :W], k
