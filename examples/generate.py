#!/usr/bin/env python3
"""Generation (greedy, or sampled on the device) from a two-layer toy decoder (token + position Embedding, pre-LayerNorm blocks of causal MultiheadAttention
and a GELU MLP, a LayerNorm and a Linear head) with incremental decoding: the prompt is prefilled in one `forward_step`, then every
new token runs through the layers alone and attends to the keys and values each layer's `KvCache` kept on the device - one read of
K and V per token instead of the causal forward over the whole prefix.

    python examples/generate.py [new_tokens]      # needs an MI355X; prints the prompt and the generated ids
    python examples/generate.py [new_tokens] --rope   # rotary positions: no position table, one shared RotaryEmbedding on every block
    python examples/generate.py [new_tokens] --rmsnorm    # the three LayerNorms become nn.RMSNorm (no centring, no bias: LLaMA's block)
    python examples/generate.py [new_tokens] --device-sample [--temperature 0.8] [--top-k 8] [--top-p 0.95] [--seed 1]
                                                      # the loop stays on the device: `nn.Sampler` draws the next ids from the logits
                                                      # where the head left them, the ids Var feeds `Embedding.forward`, and the host
                                                      # reads the ids once, after the last step.  Temperature 0 (the default) is greedy
                                                      # and generates the ids of the host path token for token
    python examples/generate.py [new_tokens] --kv-heads 2    # grouped-query attention: 4 query heads share 2 (or 1: multi-query) key /
                                                      # value heads; the caches are built with that many heads and hold 1/2 (1/4) of
                                                      # the bytes; with --rope --rmsnorm this is the attention block of LLaMA-2-70B / 3
    python examples/generate.py 240 --window 64 --rolling    # sliding-window attention (Mistral): every position attends to the last
                                                      # 64 only; --rolling keeps them in a ring of window + prompt - 1 slots per layer
                                                      # however long the generation runs (here past three times the ring); without
                                                      # --rolling the caches are linear, long enough for the whole run, and the ids
                                                      # are the same
    python examples/generate.py [new_tokens] --quant 8 [--group 32]    # weight-only quantised decoding: every step's projections read
                                                      # int8 (or --quant 4: int4) weights with per-group f32 scales (--group 32 / 64 /
                                                      # 128, default one scale per row) - `mha.quantize` for q / k / v / o,
                                                      # `nn.QuantLinear` for the MLP and the head; a twin model with the same seeds
                                                      # keeps its f32 weights, runs the same ids, and the largest difference of any
                                                      # step's logits between the two is printed (information, not a check)

The weights are random (fixed seeds): the text means nothing, the mechanics are the point.  The last lines compare every step's
logits with those of the full causal forward over the same prefix."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VOCAB, D_MODEL, HEADS, LAYERS, CONTEXT = 64, 128, 4, 2, 64


class Block:
    def __init__(self, nk, dev, seed, rope=None, norm=None, kv_heads=HEADS, window=0):
        norm = norm or nk.nn.LayerNorm
        self.ln1, self.ln2 = norm(dev, [D_MODEL]), norm(dev, [D_MODEL])
        self.mha = nk.nn.MultiheadAttention(dev, D_MODEL, HEADS, 0.0, seed, kv_heads=kv_heads)
        self.mha.causal = True
        self.mha.drop.eval()
        self.mha.rope = rope                                             # None: the learned position table below carries the positions
        self.mha.window = window                                         # 0: every position attends to its whole prefix
        self.up, self.down = nk.nn.Linear(dev, D_MODEL, 4 * D_MODEL, seed + 20), nk.nn.Linear(dev, 4 * D_MODEL, D_MODEL, seed + 22)
        self.act = nk.nn.GELU()
        self.qup = self.qdown = None

    def quantize(self, nk, bits, group):
        """the step's weights as int8 / int4 images; `full` keeps reading the f32 ones"""
        self.mha.quantize(bits, group)
        self.qup, self.qdown = nk.nn.QuantLinear(self.up, bits, group), nk.nn.QuantLinear(self.down, bits, group)

    def mlp(self, h, up=None, down=None):
        up, down = up or self.up, down or self.down
        return down.forward(self.act.forward(up.forward(self.ln2.forward(h)))) + h

    def step(self, h, batch, cache):
        """the new positions only; `cache` holds this layer's keys and values"""
        return self.mlp(self.mha.forward_step(self.ln1.forward(h), batch, cache) + h, self.qup, self.qdown)

    def full(self, h, batch):
        """every position at once: the causal forward"""
        return self.mlp(self.mha.forward(self.ln1.forward(h), batch) + h)


class Decoder:
    def __init__(self, nk, dev, rope=False, rmsnorm=False, kv_heads=HEADS, window=0, context=CONTEXT):
        self.nk, self.dev = nk, dev
        norm = nk.nn.RMSNorm if rmsnorm else nk.nn.LayerNorm
        self.tok, self.pos = nk.nn.Embedding(dev, VOCAB, D_MODEL, seed=1), nk.nn.Embedding(dev, context, D_MODEL, seed=2)
        # rotary mode: the queries and keys of every layer are rotated by their position (at lens[b] + t in a step, so the caches
        # hold rotated keys) and nothing is added to the token embedding
        self.rope = nk.nn.RotaryEmbedding(dev, D_MODEL // HEADS, context) if rope else None
        self.blocks = [Block(nk, dev, 100 * (i + 1), self.rope, norm, kv_heads, window) for i in range(LAYERS)]
        self.ln, self.head = norm(dev, [D_MODEL]), nk.nn.Linear(dev, D_MODEL, VOCAB, 7)
        self.qhead = None

    def quantize(self, bits, group):
        for block in self.blocks:
            block.quantize(self.nk, bits, group)
        self.qhead = self.nk.nn.QuantLinear(self.head, bits, group)

    def embed(self, ids, first, shape=None):
        """ids (batch, T) at positions first .. first + T - 1 -> (batch * T, d_model); a device Var of batch * T ids comes with its
        `shape` = (batch, T) and is gathered where it is"""
        batch, T = ids.shape if shape is None else shape
        where = np.tile(np.arange(first, first + T, dtype=np.float32), batch)
        up = lambda a: self.nk.from_ndarray(self.dev, np.ascontiguousarray(a, dtype=np.float32).reshape(-1))
        tokens = self.tok.forward(up(ids) if shape is None else ids)
        if self.rope is not None:
            return tokens
        return tokens + self.pos.forward(up(where))

    def step(self, ids, first, caches, shape=None):
        """the logits of the new positions as a (batch * T, vocab) variable on the device, computed"""
        batch = ids.shape[0] if shape is None else shape[0]
        h = self.embed(ids, first, shape)
        for block, cache in zip(self.blocks, caches):
            h = block.step(h, batch, cache)
        out = (self.qhead or self.head).forward(self.ln.forward(h))
        out.forward()
        return out

    def logits_step(self, ids, first, caches):
        return self.step(ids, first, caches).data().reshape(ids.shape[0], ids.shape[1], VOCAB)

    def logits_full(self, ids):
        h = self.embed(ids, 0)
        for block in self.blocks:
            h = block.full(h, ids.shape[0])
        out = self.head.forward(self.ln.forward(h))
        out.forward()
        return out.data().reshape(ids.shape[0], ids.shape[1], VOCAB)


def generate_on_device(nk, dev, model, prompt, new_tokens, caches, temperature, top_k, top_p, seed):
    """The loop without the host: every step's logits stay where the head wrote them, `nn.Sampler` draws the next id of each sample
    from their last row, and that (batch,) Var is the next step's input.  One read of the ids behind the last step.  (Each step's
    graph keeps the earlier steps' nodes in its history; they were computed once and are not run again.)"""
    batch, n = prompt.shape
    sampler = nk.nn.Sampler(dev, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed)
    logits = model.step(prompt, 0, caches)                               # prefill
    drawn = []
    for i in range(new_tokens):
        nxt = sampler.forward(logits, batch)                             # (batch,) ids as f32, no gradient
        drawn.append(nxt)
        logits = model.step(nxt, n + i, caches, shape=(batch, 1))
    assert sampler.offset == new_tokens                                  # one Philox offset per executed draw
    new = np.stack([v.data() for v in drawn], axis=1).astype(prompt.dtype)
    ids = np.concatenate([prompt, new], axis=1)
    worst = float(np.abs(logits.data().reshape(batch, VOCAB) - model.logits_full(ids)[:, -1]).max())
    return ids, worst


def main(new_tokens=16, rope=False, device_sample=False, temperature=0.0, top_k=0, top_p=1.0, seed=0, rmsnorm=False, kv_heads=HEADS, window=0,
         rolling=False, quant=0, group=0):
    import neuronika_amd
    nk = neuronika_amd.tape
    dev = nk.Device(0)
    prompt = np.array([[3, 14, 15, 9, 26, 5, 35, 8]])
    batch, n = prompt.shape
    context = max(CONTEXT, n + new_tokens)                               # positions the run reaches: the position table / rope table
    assert window > 0 or not rolling, "--rolling keeps the last positions only: it needs --window"
    assert window > 0 or context == CONTEXT, "more than %d positions need --window" % CONTEXT
    model = Decoder(nk, dev, rope, rmsnorm, kv_heads, window, context)
    # a linear cache holds every position of the run; a rolling one the window and the prompt's rows, whatever the length
    slots, ring = (window + n - 1, dict(rolling=True)) if rolling else (context, dict())
    new_caches = lambda: [nk.nn.KvCache(dev, batch, kv_heads, D_MODEL // HEADS, slots, **ring) for _ in range(LAYERS)]   # kv_heads heads per layer
    caches = new_caches()
    twin, apart = None, 0.0
    if quant:
        assert not device_sample, "--quant compares every step with an f32 twin on the host path"
        model.quantize(quant, group)
        twin, twin_caches = Decoder(nk, dev, rope, rmsnorm, kv_heads, window, context), new_caches()   # same seeds, f32 weights
    if device_sample:
        ids, worst = generate_on_device(nk, dev, model, prompt, new_tokens, caches, temperature, top_k, top_p, seed)
    else:
        logits = model.logits_step(prompt, 0, caches)                    # prefill: every prompt position in one step
        if twin:
            apart = float(np.abs(logits - twin.logits_step(prompt, 0, twin_caches)).max())
        ids, worst = prompt, 0.0
        for _ in range(new_tokens):
            nxt = logits[:, -1].argmax(axis=1).reshape(batch, 1)
            ids = np.concatenate([ids, nxt], axis=1)
            logits = model.logits_step(nxt, ids.shape[1] - 1, caches)    # one token through the layers, K and V from the caches
            if twin:
                apart = max(apart, float(np.abs(logits - twin.logits_step(nxt, ids.shape[1] - 1, twin_caches)).max()))
            worst = max(worst, float(np.abs(logits[:, -1] - model.logits_full(ids)[:, -1]).max()))
    assert caches[0].lens() == [n + new_tokens] * batch
    if rolling:
        print("rolling caches of %d slots held the last %d of %d positions" % (slots, window, n + new_tokens))
    print("prompt   ", prompt[0].tolist())
    print("generated", ids[0, n:].tolist())
    print("largest difference between a step's logits and the full causal forward's: %.3g" % worst)
    if twin:
        print("int%d weights (group %s): largest difference of a step's logits from the f32 model's on the same ids: %.3g"
              % (quant, group or "row", apart))
    return ids, worst


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("new_tokens", nargs="?", type=int, default=16)
    ap.add_argument("--rope", action="store_true", help="rotary positions instead of the learned position table")
    ap.add_argument("--rmsnorm", action="store_true", help="nn.RMSNorm in place of the three nn.LayerNorm")
    ap.add_argument("--kv-heads", type=int, default=HEADS, choices=[1, 2, 4], help="key / value heads shared by the %d query heads (grouped-query attention)" % HEADS)
    ap.add_argument("--window", type=int, default=0, help="sliding-window attention: every position attends to the last WINDOW positions (0 = off)")
    ap.add_argument("--rolling", action="store_true", help="with --window: rolling caches of window + prompt - 1 slots instead of linear ones")
    ap.add_argument("--device-sample", action="store_true", help="draw the next ids on the device (nn.Sampler); the host reads them once")
    ap.add_argument("--temperature", type=float, default=0.0, help="with --device-sample: 0 = greedy")
    ap.add_argument("--top-k", type=int, default=0, help="with --device-sample: 0 = off")
    ap.add_argument("--top-p", type=float, default=1.0, help="with --device-sample: 1 = off")
    ap.add_argument("--seed", type=int, default=0, help="with --device-sample: the Philox key of the draws")
    ap.add_argument("--quant", type=int, default=0, choices=[0, 8, 4], help="weight-only quantised decoding: int8 or int4 weights in every step (0 = off)")
    ap.add_argument("--group", type=int, default=0, choices=[0, 32, 64, 128], help="with --quant: weights per f32 scale (0 = one scale per row)")
    a = ap.parse_args()
    main(a.new_tokens, rope=a.rope, device_sample=a.device_sample, temperature=a.temperature, top_k=a.top_k, top_p=a.top_p, seed=a.seed, rmsnorm=a.rmsnorm,
         kv_heads=a.kv_heads, window=a.window, rolling=a.rolling, quant=a.quant, group=a.group)
