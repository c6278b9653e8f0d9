"""nk_embedding_* at the sizes of real models, bit for bit against tests/embedding_oracle.py: GPT-2 small's table (50 257 x 768)
with 8 x 1024 tokens, and a 32 000 x 4096 table with 16 384 tokens; uniform and Zipf-distributed ids."""
import numpy as np
import pytest

import embedding_oracle as E
from test_gpu_embedding import same_bits, uniform_ids, zipf_ids

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("V,D,n", [(50257, 768, 8 * 1024), (32000, 4096, 16384)])
@pytest.mark.parametrize("ids", (uniform_ids, zipf_ids))
def test_model_sizes(dev, V, D, n, ids):
    from neuronika_amd import capi as c
    rng = np.random.default_rng(V + n)
    idx = ids(rng, n, V)
    if ids is zipf_ids:
        assert np.bincount(idx.astype(np.int64)).max() > E.CHUNK          # the most frequent token's row is summed in chunks
    weight = rng.standard_normal((V, D), dtype=np.float32)
    g = rng.standard_normal((n, D), dtype=np.float32)
    W, I, G = dev.array(weight), dev.array(idx), dev.array(g)
    OUT = dev.full((n, D), np.nan)
    c.embedding_fwd(dev, W, I, OUT, n, V, D)
    same_bits(OUT.numpy(), weight[idx.astype(np.int64)], "forward")
    del OUT
    want = E.backward_assign(g, idx, V)
    DA = dev.full((V, D), np.nan)
    c.embedding_bwd(dev, DA, G, I, n, V, D, assign=True)
    same_bits(DA.numpy(), want, "backward assign")
    del DA
    c.embedding_bwd(dev, W, G, I, n, V, D)                                  # += onto the table itself: a non-zero destination
    touched = np.zeros(V, bool)
    touched[idx.astype(np.int64)] = True
    weight[touched] = weight[touched] + want[touched]
    same_bits(W.numpy(), weight, "backward +=")
