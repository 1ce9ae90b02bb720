"""The shared helpers of tests/gpu_world.py on the CPU: the packing round trip, host edits in order, and the
sparse worlds -- whose bits must stay what the tests received while every module carried its own generator."""
import hashlib

import numpy as np
import pytest

from gpu_world import dims, edited, pack, sparse_bits, voxels

# SHA-256 of the bit words for every (lg, density, seed) the tests pass.  Computed with the generators of
# the commit before the helpers were shared (test_gpu_world_edit._sparse_bits, which
# test_world_scroll_region.sparse_bits equalled, and test_gpu_gi_relight._sparse_bits), not with gpu_world.
EXACT = {
    ((10, 6, 6), 1e-06, 77): "5cf8b3b951535816835de8daffe2ac154235aa542e9476cd41d263371d31f84e",
    ((6, 10, 6), 1e-06, 78): "a94e701f58a2a54f6b38611cc1f5f41975bfd47d35b25b3db71048d21dfc0581",
    ((6, 6, 10), 1e-06, 79): "af0cbac607ee87afd84861c27016955e1016236f8b8c316fe537dd8b1e50d53b",
    ((8, 8, 8), 2e-05, 31): "b8f44166a0ec9c09703cc9fbd0ae42288831bf6efc12ba9cd07b288ca7826b12",
    ((7, 9, 7), 2e-05, 32): "a2d704b4db2c8d63b509df41b0b420f36d6c66b059013f2a5139cc3798bcc5aa",
    ((7, 7, 9), 2e-05, 33): "d08021e0006a5c964512d7ed53989184fb06db3bb5945660cd5705fbf0bdd51d",
    ((10, 6, 6), 2e-05, 31): "ec8f018c5cc5cbd82e2064aedbcecb6fef1d16854270fe1c9f0357bb284dade9",
    ((6, 6, 10), 2e-05, 33): "0695f49674c29661a9c7f6fe5418f02133c72662774f9a4c88b5007c4836e779",
    ((10, 6, 6), 1e-06, 1119): "fd06cb4a8a6d86153c5988cf4f86cbcc0a777e2132d0af58ab0753204aa57241",
    ((10, 6, 6), 1e-06, 1036): "98b8c44fb5dfc45a5f28cc7871e0cdede971c590ecdda665264eb398e3d20f42",
    ((10, 6, 6), 1e-06, 1005): "e6274360bf23f5e2fc69a5f1b936afaf953e87073a88d3af38be08e0efa4a348",
    ((10, 6, 6), 1e-06, 1049): "b67575d1b9517cfb72d51b7b5aab6448de0f96e72f89b5ce55baa5766c98b589",
    ((6, 6, 10), 1e-06, 1036): "98b8c44fb5dfc45a5f28cc7871e0cdede971c590ecdda665264eb398e3d20f42",
    ((6, 6, 10), 1e-06, 1074): "011c90f769140cc474ceed18c82ce770e46adb3bedfe5114d4bc8367ea12e1f4",
    ((6, 6, 10), 1e-06, 1009): "522b5e898ebde713dc9b90de692a4fcf6a84a289bb09ed10999b89a87bc11245",
    ((6, 6, 10), 1e-06, 1037): "be8d1a95877aeda968b9312a788b54431dc0de816b35f4d8e466b33a3f8147b5",
    ((10, 6, 6), 1e-06, 1060): "49d6296a95889f5d69764e5105fcc3108375f7bb1812703b77350aa4ec2fa7e3",
    ((6, 6, 10), 1e-06, 1027): "f4ad11f5c441b7ba6d5084a5915cd4e16649f2e73a3a24c5dfe0d3bfd587edb5",
    ((10, 6, 6), 0.0, 107): "07854d2fef297a06ba81685e660c332de36d5d18d546927d30daad6d7fda1541",
    ((10, 6, 6), 0.0001, 107): "f9f5792c41b4c065369a17ac20690bde0ada113d17737e60703051ac9fe9a2e6",
    ((10, 6, 6), 0.0, 139): "07854d2fef297a06ba81685e660c332de36d5d18d546927d30daad6d7fda1541",
    ((10, 6, 6), 0.0001, 139): "dc2805972c2f8493d3ee54676542694ea52336170c8c0c9739dfc6830007d1c8",
    ((10, 6, 6), 0.0, 163): "07854d2fef297a06ba81685e660c332de36d5d18d546927d30daad6d7fda1541",
    ((10, 6, 6), 0.0001, 163): "33e68d9cfbd6ace049cd0cbbed54f9081595fa30b31b4c6c0d6446f5173f4cae",
    ((6, 6, 10), 0.0, 109): "07854d2fef297a06ba81685e660c332de36d5d18d546927d30daad6d7fda1541",
    ((6, 6, 10), 0.0001, 109): "c6f0c0726acee9bbc82deec6913bba27a7656aa74d30868f1a5d1e228e44f73f",
    ((6, 6, 10), 0.0, 141): "07854d2fef297a06ba81685e660c332de36d5d18d546927d30daad6d7fda1541",
    ((6, 6, 10), 0.0001, 141): "235c6522fc75178e6d4f65e14ee0caa6f508894dcfaacfb95f2bb3ad2082be38",
    ((6, 6, 10), 0.0, 165): "07854d2fef297a06ba81685e660c332de36d5d18d546927d30daad6d7fda1541",
    ((6, 6, 10), 0.0001, 165): "47e2c93fa657075bab8d2f227b6919e5f96143d77a94f4828d9e06b1fd9cc52e",
}
DRAWN = {   # exact=False: int(n * density) draws with replacement
    ((4, 4, 4), 0.1, 5): "8af86d68d6f8abda594fc8d725c5e2152713118eeb3482ca343791bc373cdc6b",
    ((6, 6, 6), 0.05, 3): "03e65623c57bc51d85b3325ad2fba1173908a977f3a255134e5ce4f659f073c3",
    ((7, 5, 6), 0.03, 3): "b8b72481698303614ee365861bc4b0ca98a35acf6fce85fb4b89b6d1b336ed88",
}


@pytest.mark.parametrize("lg", [(4, 4, 4), (5, 4, 6)])
def test_pack_and_voxels_round_trip(lg):
    X, Y, Z = dims(lg)
    bits = np.random.default_rng(sum(lg)).integers(0, 2 ** 32, X * Y * Z // 32, dtype=np.uint32)
    vox = voxels(bits, lg)
    assert vox.shape == (Z, Y, X) and vox.dtype == bool
    assert np.array_equal(pack(vox), bits)
    # bit i of the words is voxel x | y << lx | z << (lx + ly)
    x, y, z = 3, Y - 1, Z - 2
    i = x | (y << lg[0]) | (z << (lg[0] + lg[1]))
    assert vox[z, y, x] == bool((bits[i >> 5] >> (i & 31)) & 1)
    one = np.zeros_like(vox)
    one[z, y, x] = True
    assert np.flatnonzero(pack(one)).tolist() == [i >> 5] and int(pack(one)[i >> 5]) == 1 << (i & 31)


def test_edited_applies_overlapping_boxes_in_order():
    lg = (5, 4, 6)
    X, Y, Z = dims(lg)
    bits = np.zeros(X * Y * Z // 32, np.uint32)
    boxes = [(1, 2, 3, 20, 12, 30, 1), (5, 0, 10, 9, 16, 20, 0), (7, 4, 15, 8, 5, 40, 1)]
    vox = voxels(edited(bits, lg, boxes), lg)
    want = np.zeros((Z, Y, X), bool)
    want[3:30, 2:12, 1:20] = True
    want[10:20, 0:16, 5:9] = False
    want[15:40, 4:5, 7:8] = True
    assert np.array_equal(vox, want)
    assert vox[16, 4, 7] and not vox[16, 4, 6] and vox[16, 4, 4]      # set over clear over set
    assert not np.array_equal(edited(bits, lg, boxes[::-1]), pack(want))   # the order matters
    assert not bits.any()                                              # the input is left alone
    assert np.array_equal(edited(pack(want), lg, []), pack(want))


def test_sparse_worlds_are_the_ones_the_tests_had():
    for (lg, density, seed), want in EXACT.items():
        bits = sparse_bits(lg, density, seed)
        assert hashlib.sha256(bits.tobytes()).hexdigest() == want, (lg, density, seed)
        assert int(np.unpackbits(bits.view(np.uint8)).sum()) == int(round((1 << sum(lg)) * density))
    for (lg, density, seed), want in DRAWN.items():
        bits = sparse_bits(lg, density, seed, exact=False)
        assert hashlib.sha256(bits.tobytes()).hexdigest() == want, (lg, density, seed)
        assert 0 < int(np.unpackbits(bits.view(np.uint8)).sum()) <= int((1 << sum(lg)) * density)
