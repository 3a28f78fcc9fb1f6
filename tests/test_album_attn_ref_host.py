"""tests/_album_attn_ref.py restates the album attention once, over the pooled form, and serves the shared-context family
through `as_pooled`: shared = pooled at M = 1.  That claim, pinned on the two families' DEFINITIONS (which do not go
through the restatements): the pool's definition on the adapted case gives the shared definition's forward bit for bit --
the same values through the same oracle calls -- and its gradients to fp64 rounding, d_pool against d_h.  No GPU."""
import torch

from tests import _album_attn_ref as AR
from tests import _attn_pool_bwd_ref as PB
from tests import _attn_pool_tw_bwd_ref as PTB
from tests import _attn_shared_bwd_ref as B
from tests import _attn_shared_ref as R
from tests import _attn_shared_tw_bwd_ref as TB
from tests import _attn_shared_tw_ref as TW


def test_shared_definition_is_the_pooled_one_at_one_album_per_question():
    # A = 3, NQ = 4: album 1 without a question, albums 0 and 2 with two each; K 2, T 5, JQ 3, w 8; simiMatrix 2 with tanh,
    # masked; warp type 5, window 1.0
    c = TW.add_warp(R.train_recipe([2, 0, 2], 2, 5, 3, 8, 2, True, True, 7), 7, 5, 1.0)
    assert sorted(torch.bincount(c["album"], minlength=3).tolist()) == [0, 2, 2] and (c["A"], c["NQ"]) == (3, 4)
    p = AR.as_pooled(c)
    assert p["pool"] is c["h"] and p["pm"] is c["hm"]                                   # views, not copies
    assert p["albums"].data_ptr() == c["album"].data_ptr() and (p["P"], p["M"], p["JX"]) == (3, 1, 5)
    for shared, pooled, forward in ((TB.reference(c), PTB.reference(p), ("h_a", "a_logits", "scale")),
                                    (B.reference(c), PB.reference(p), ("h_a", "a_logits"))):
        assert set(AR.as_shared(pooled)) == set(shared)
        for k in forward:
            assert torch.equal(pooled[k], shared[k]), k
        grads = [k for k in shared if k not in forward]
        assert len(grads) == 9 - 5 * (len(forward) == 2) and "dh" in grads
        for k in grads:
            # fp64 sums of at most NQ = 4 terms taken in another order: about 1e-15, three orders of headroom
            want, got = shared[k], AR.as_shared(pooled)[k]
            err = float((got - want).abs().max())
            assert err <= 1e-12 * max(1.0, float(want.abs().max())), (k, err)
