"""The category limits of the kernels on resident partials and k_edge's LDS bytes, pinned value
for value: every *Lds struct shares one head (ModelLds) and every limit one loop
(max_cat of pu_resident.h), so a byte moved in either shows here.  Host code only: no device."""
import ctypes

import pytest

from phylo_utils_amd import _native as N

# K: (2, 4, 20)
MAX_CAT = {
    "pu_quartet_max_cat": (25, 24, 19),    # the LDS alone (no context can hold more than 64)
    "pu_ancestral_max_cat": (64, 50, 10),
    "pu_counts_max_cat": (64, 64, 6),
    "pu_place_max_cat": (64, 49, 10),      # K = 20: also C K <= 256
    "pu_regraft_max_cat": (64, 64, 20),
}
# (mode, K): bytes at C = 1 and C = 4; modes EDGE_UPDATE, EDGE_LNL, EDGE_DERIV
EDGE_LDS = {
    (0, 2): (384, 688), (0, 4): (816, 1792), (0, 20): (13488, 33664),
    (1, 2): (896, 2736), (1, 4): (1328, 3840), (1, 20): (14000, 35712),
    (2, 2): (2528, 9264), (2, 4): (3184, 11264), (2, 20): (22256, 68736),
}


@pytest.mark.parametrize("name", sorted(MAX_CAT))
def test_max_cat_values(name):
    fn = getattr(N.lib(), name)
    assert tuple(fn(K) for K in (2, 4, 20)) == MAX_CAT[name]
    for K in (0, 3, 7, 21):
        assert fn(K) == N.PU_E_ARG


def test_edge_lds_bytes():
    fn = getattr(N.lib(), "_ZN2pu14edge_lds_bytesEiii")  # pu::edge_lds_bytes(int, int, int)
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_int] * 3
    for (mode, K), want in EDGE_LDS.items():
        assert (fn(mode, K, 1), fn(mode, K, 4)) == want
