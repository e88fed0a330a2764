"""Which kernel a dense product or a prefill attention reaches, as the library answers it: `gemm_route` / `attn_route` call amt_gemm_route /
amt_attn_route, which evaluate the very functions `amt_launch_gemm` and `launch_hd` branch on (host code, no GPU).  BOUNDARIES is the one
place the tests write the present thresholds down; test_train_edges_host.py::test_launch_boundaries_are_the_librarys proves each entry."""
from collections import namedtuple

from video2music_amd.ops import attn_route, gemm_route      # noqa: F401  'rows128' | 'splitk';  'skinny' | 'tile64' | 'tile128'

# more rows (small_m), more outputs (small_mn) or a longer K (skinny_k) leave the skinny GEMM; fewer 128x128 tiles (t64_below) or a shorter K
# (big_k) take the 64-tile kernel; the split-key kernel serves grids below split_grid workgroups of attn_row_block query rows with at least
# split_lk keys, at the head dims split_hd, without a relative position table
BOUNDARIES = dict(small_m=4096, small_mn=650000, skinny_k=1536, t64_below=768, big_k=2048,
                  attn_row_block=128, split_grid=512, split_lk=256, split_hd=(32, 64))

# one dense product as the forward issues it; other_forms: a head-split, row-addend, silu-multiply, grouped or gathered product
GemmCall = namedtuple("GemmCall", "name M N K act other_forms")


def route_of(q):
    """The GEMM route of a GemmCall, or of a helpers_ops_edges.GemmCase (which has no other_forms: the C ABI sets none)."""
    return gemm_route(q.M, q.N, q.K, q.act, getattr(q, "other_forms", False))


def vec_ok(N, ldc, ldr=None):
    """vec_ok of gemm_f32_kernel for a product through the C ABI (ldr: the residual's, None without one): 16-byte stores, else element-wise
    ones.  Decided inside the tiled kernels, so it stays a restatement; the skinny kernel has one element-wise epilogue and is not asked."""
    return N % 4 == 0 and ldc % 4 == 0 and (ldr is None or ldr % 4 == 0)
