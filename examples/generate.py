#!/usr/bin/env python3
"""Greedy generation from a two-layer toy decoder (token + position Embedding, pre-LayerNorm blocks of causal MultiheadAttention
and a GELU MLP, a LayerNorm and a Linear head) with incremental decoding: the prompt is prefilled in one `forward_step`, then every
new token runs through the layers alone and attends to the keys and values each layer's `KvCache` kept on the device - one read of
K and V per token instead of the causal forward over the whole prefix.

    python examples/generate.py [new_tokens]      # needs an MI355X; prints the prompt and the generated ids
    python examples/generate.py [new_tokens] --rope   # rotary positions: no position table, one shared RotaryEmbedding on every block

The weights are random (fixed seeds): the text means nothing, the mechanics are the point.  The last lines compare every step's
logits with those of the full causal forward over the same prefix."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VOCAB, D_MODEL, HEADS, LAYERS, CONTEXT = 64, 64, 2, 2, 64


class Block:
    def __init__(self, nk, dev, seed, rope=None):
        self.ln1, self.ln2 = nk.nn.LayerNorm(dev, [D_MODEL]), nk.nn.LayerNorm(dev, [D_MODEL])
        self.mha = nk.nn.MultiheadAttention(dev, D_MODEL, HEADS, 0.0, seed)
        self.mha.causal = True
        self.mha.drop.eval()
        self.mha.rope = rope                                             # None: the learned position table below carries the positions
        self.up, self.down = nk.nn.Linear(dev, D_MODEL, 4 * D_MODEL, seed + 20), nk.nn.Linear(dev, 4 * D_MODEL, D_MODEL, seed + 22)
        self.act = nk.nn.GELU()

    def mlp(self, h):
        return self.down.forward(self.act.forward(self.up.forward(self.ln2.forward(h)))) + h

    def step(self, h, batch, cache):
        """the new positions only; `cache` holds this layer's keys and values"""
        return self.mlp(self.mha.forward_step(self.ln1.forward(h), batch, cache) + h)

    def full(self, h, batch):
        """every position at once: the causal forward"""
        return self.mlp(self.mha.forward(self.ln1.forward(h), batch) + h)


class Decoder:
    def __init__(self, nk, dev, rope=False):
        self.nk, self.dev = nk, dev
        self.tok, self.pos = nk.nn.Embedding(dev, VOCAB, D_MODEL, seed=1), nk.nn.Embedding(dev, CONTEXT, D_MODEL, seed=2)
        # rotary mode: the queries and keys of every layer are rotated by their position (at lens[b] + t in a step, so the caches
        # hold rotated keys) and nothing is added to the token embedding
        self.rope = nk.nn.RotaryEmbedding(dev, D_MODEL // HEADS, CONTEXT) if rope else None
        self.blocks = [Block(nk, dev, 100 * (i + 1), self.rope) for i in range(LAYERS)]
        self.ln, self.head = nk.nn.LayerNorm(dev, [D_MODEL]), nk.nn.Linear(dev, D_MODEL, VOCAB, 7)

    def embed(self, ids, first):
        """ids (batch, T) at positions first .. first + T - 1 -> (batch * T, d_model)"""
        batch, T = ids.shape
        where = np.tile(np.arange(first, first + T, dtype=np.float32), batch)
        up = lambda a: self.nk.from_ndarray(self.dev, np.ascontiguousarray(a, dtype=np.float32).reshape(-1))
        if self.rope is not None:
            return self.tok.forward(up(ids))
        return self.tok.forward(up(ids)) + self.pos.forward(up(where))

    def logits_step(self, ids, first, caches):
        h = self.embed(ids, first)
        for block, cache in zip(self.blocks, caches):
            h = block.step(h, ids.shape[0], cache)
        out = self.head.forward(self.ln.forward(h))
        out.forward()
        return out.data().reshape(ids.shape[0], ids.shape[1], VOCAB)

    def logits_full(self, ids):
        h = self.embed(ids, 0)
        for block in self.blocks:
            h = block.full(h, ids.shape[0])
        out = self.head.forward(self.ln.forward(h))
        out.forward()
        return out.data().reshape(ids.shape[0], ids.shape[1], VOCAB)


def main(new_tokens=16, rope=False):
    import neuronika_amd
    nk = neuronika_amd.tape
    dev = nk.Device(0)
    model = Decoder(nk, dev, rope)
    prompt = np.array([[3, 14, 15, 9, 26, 5, 35, 8]])
    batch, n = prompt.shape
    assert n + new_tokens <= CONTEXT
    caches = [nk.nn.KvCache(dev, batch, HEADS, D_MODEL // HEADS, CONTEXT) for _ in range(LAYERS)]
    logits = model.logits_step(prompt, 0, caches)                        # prefill: every prompt position in one step
    ids, worst = prompt, 0.0
    for _ in range(new_tokens):
        nxt = logits[:, -1].argmax(axis=1).reshape(batch, 1)
        ids = np.concatenate([ids, nxt], axis=1)
        logits = model.logits_step(nxt, ids.shape[1] - 1, caches)        # one token through the layers, K and V from the caches
        worst = max(worst, float(np.abs(logits[:, -1] - model.logits_full(ids)[:, -1]).max()))
    assert caches[0].lens() == [n + new_tokens] * batch
    print("prompt   ", prompt[0].tolist())
    print("generated", ids[0, n:].tolist())
    print("largest difference between a step's logits and the full causal forward's: %.3g" % worst)
    return ids, worst


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--rope"]
    main(int(args[0]) if args else 16, rope="--rope" in sys.argv[1:])
