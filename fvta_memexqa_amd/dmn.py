"""The DMN+ episodic memory the AttentionGRUCell lives in (reference model_dmnplus.py:503-516 around
`_generate_episode` :113-136 and `_get_attention` :89-111), forward AND backward:

    prev_memory = gq
    for i in range(num_hops):
        episode = _generate_episode(prev_memory, gq, facts, facts_length, i, d)       # attention MLP -> softmax over
        prev_memory = relu(dense(concat([prev_memory, episode, gq], 1), d))           # the facts -> AttentionGRU over them
    output = prev_memory

Every hop shares the attention MLP and the AttentionGRU (the reference's reuse flags, :117, :123); each hop has its own
dense layer ("hop_%d").  All arithmetic runs in the HIP library (feature vector, linears, softmax, the gated recurrence
over all facts in one fvta_attgru_seq_fwd, relu).  The class is a shell with explicit `params` / `grads` dictionaries over
the library's one differentiable hop loop (functional.episodic_memory_raw, which nn.EpisodicMemory and
functional.episodic_memory run too): `forward` records the autograd graph, `backward` walks it (and may walk it
again) and ADDS the parameter gradients into `grads`.  What the reference builds AROUND this module in the DMN+
model -- uni-directional encoders, the bi-GRU fusion of the facts, its own output layer (model_dmnplus.py:300-500,
:518-560) -- is not built: DESIGN.md section 7.

Variable names are TensorFlow's (tf.contrib.layers.fully_connected: weights/biases; tf.layers.dense: kernel/bias;
dynamic_rnn adds "rnn"): memory/attention/fc{1,2}/{weights,biases},
memory/attention_gru/rnn/attention_gru_cell/{gates,candidate,input}/{weights[,biases]}, memory/hop_<i>/dense/{kernel,bias}.
"""
import torch

from . import functional, ops

CELL = "memory/attention_gru/rnn/attention_gru_cell/"
CELL_VARS = functional._CELL_VARS
ATT_VARS = ("memory/attention/fc1/weights", "memory/attention/fc1/biases", "memory/attention/fc2/weights",
            "memory/attention/fc2/biases")


def init_params(hidden_size, num_hops, seed=0):
    """The 9 + 2 * num_hops variables under their TF names, on the CPU: Glorot uniform weights drawn in this order from one
    generator, zero biases (bias_start 0.0, attention_gru_cell.py:72)."""
    d = int(hidden_size)
    g = torch.Generator().manual_seed(seed)

    def glorot(fi, fo):
        lim = (6.0 / (fi + fo)) ** 0.5
        return (torch.rand(fi, fo, generator=g) * 2 - 1) * lim

    p = {ATT_VARS[0]: glorot(4 * d, d), ATT_VARS[1]: torch.zeros(d), ATT_VARS[2]: glorot(d, 1), ATT_VARS[3]: torch.zeros(1)}
    for name, shape in CELL_VARS:
        sh = shape(d)
        p[CELL + name] = torch.zeros(*sh) if name.endswith("biases") else glorot(*sh)
    for i in range(int(num_hops)):
        p["memory/hop_%d/dense/kernel" % i] = glorot(3 * d, d)
        p["memory/hop_%d/dense/bias" % i] = torch.zeros(d)
    return p


def split_params(p, num_hops, prefix="memory/"):
    """(att_vars, cell_vars, hop_vars) of functional.episodic_memory_raw out of a name -> tensor mapping"""
    cell = prefix + CELL[len("memory/"):]
    return (tuple(p[prefix + k[len("memory/"):]] for k in ATT_VARS), tuple(p[cell + name] for name, _ in CELL_VARS),
            [(p[prefix + "hop_%d/dense/kernel" % i], p[prefix + "hop_%d/dense/bias" % i]) for i in range(int(num_hops))])


class EpisodicMemory:
    def __init__(self, hidden_size, num_hops, device="cuda", seed=0):
        ops.require_gpu()
        self.d, self.num_hops, self.device = int(hidden_size), int(num_hops), torch.device(device)
        self.params = {k: v.to(self.device) for k, v in init_params(self.d, self.num_hops, seed).items()}
        self.grads = {k: torch.zeros_like(v) for k, v in self.params.items()}
        self._saved = None

    # ------------------------------------------------------------------ weights
    def set_weights(self, weights):
        for k, v in weights.items():
            if k not in self.params:
                raise KeyError(k)
            t = torch.as_tensor(v, dtype=torch.float32).reshape(self.params[k].shape)
            self.params[k].copy_(t)

    def zero_grad(self):
        for gr in self.grads.values():
            gr.zero_()

    # ------------------------------------------------------------------ forward
    def forward(self, gq, facts, facts_length):
        """gq [N,d] (the question vector, also the first memory), facts [N,F,d], facts_length [N] -> output [N,d]."""
        d = self.d
        gq = gq.to(self.device, torch.float32).contiguous()
        facts = facts.to(self.device, torch.float32).contiguous()
        N = facts.shape[0]
        if gq.shape != (N, d) or facts.shape[2] != d:
            raise ValueError("EpisodicMemory: gq %s / facts %s do not fit hidden size %d" % (tuple(gq.shape), tuple(facts.shape), d))
        # leaves of this call's graph: views of the inputs and of `params` (shared storage, no copy)
        leaves = {k: v.detach().requires_grad_() for k, v in self.params.items()}
        gq_l, facts_l = gq.detach().requires_grad_(), facts.detach().requires_grad_()
        with torch.enable_grad():
            out = functional.episodic_memory_raw(gq_l, facts_l, facts_length, *split_params(leaves, self.num_hops))
        self._saved = (out, gq_l, facts_l, leaves)
        return out.detach()

    __call__ = forward

    # ----------------------------------------------------------------- backward
    def backward(self, d_output):
        """Gradient of the last forward: returns (d_gq [N,d], d_facts [N,F,d]); parameter gradients are ADDED to self.grads."""
        if self._saved is None:
            raise RuntimeError("EpisodicMemory.backward before forward")
        out, gq_l, facts_l, leaves = self._saved
        names = list(leaves)
        gs = torch.autograd.grad(out, [gq_l, facts_l] + [leaves[k] for k in names],
                                 d_output.to(self.device, torch.float32).contiguous(), retain_graph=True, allow_unused=True)
        for k, g in zip(names, gs[2:]):
            if g is not None:
                self.grads[k] += g
        return gs[0], gs[1]
