"""CPU oracle for the HuBERT stage (moditalker_amd/csrc/hubert.hip behind moditalker_amd.HubertModel).  TEST INFRASTRUCTURE ONLY.

Plain torch, any dtype (float64 by default), no transformers import: the stable-layer-norm, layer-normed-conv HuBERT forward
written out from its arithmetic, as a function of a state dict with HubertModel's keys and a config with HubertModel's
keywords.  Pinned: tests/test_hubert_oracle_host.py reproduces every array of tests/golden/hubert.npz (transformers' own
outputs) within the bar stored beside it."""
import torch
import torch.nn.functional as F


def num_frames(n_samples, conv_kernel, conv_stride):
    """Frames of a clip: (n - k) // s + 1 through every conv layer; 0 when a layer has no valid window."""
    n = int(n_samples)
    for k, s in zip(conv_kernel, conv_stride):
        if n < k:
            return 0
        n = (n - k) // s + 1
    return n


def normalize(x, dtype=torch.float64):
    """Wav2Vec2FeatureExtractor's do_normalize over one utterance: (x - mean) / sqrt(var + 1e-7), biased variance."""
    x = torch.as_tensor(x).to(dtype)
    return (x - x.mean()) / torch.sqrt(x.var(unbiased=False) + 1e-7)


def hubert_forward(sd, cfg, wave, dtype=torch.float64, taps=None):
    """wave [B, n] -> last_hidden_state [B, T, hidden].  `taps` (a dict) receives extract_features, after_pos_conv and
    layer_0, each [B T, C]."""
    w = lambda key: sd[key].detach().to(device="cpu", dtype=dtype)
    ln = lambda x, pre, eps: F.layer_norm(x, x.shape[-1:], w(pre + ".weight"), w(pre + ".bias"), eps)
    lin = lambda x, pre: F.linear(x, w(pre + ".weight"), w(pre + ".bias"))
    flat = lambda t: t.reshape(-1, t.shape[-1]).clone()
    hidden, heads, eps = cfg["hidden_size"], cfg["num_attention_heads"], cfg["layer_norm_eps"]
    k_pos, groups = cfg["num_conv_pos_embeddings"], cfg["num_conv_pos_embedding_groups"]
    x = wave.detach().to(device="cpu", dtype=dtype)[:, None, :]                       # [B, 1, n]
    for i, stride in enumerate(cfg["conv_stride"]):                                   # conv -> LayerNorm over channels (1e-5) -> GELU
        pre = f"feature_extractor.conv_layers.{i}"
        x = F.conv1d(x, w(pre + ".conv.weight"), w(pre + ".conv.bias"), stride=stride)
        x = F.gelu(ln(x.transpose(1, 2), pre + ".layer_norm", 1e-5)).transpose(1, 2)
    x = x.transpose(1, 2)                                                             # [B, T, C]
    if taps is not None:
        taps["extract_features"] = flat(x)
    x = lin(ln(x, "feature_projection.layer_norm", eps), "feature_projection.projection")
    pc = "encoder.pos_conv_embed.conv"
    g, v = w(pc + ".parametrizations.weight.original0"), w(pc + ".parametrizations.weight.original1")
    wpos = v * (g / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())                    # weight_norm(dim=2): one norm per tap
    p = F.conv1d(x.transpose(1, 2), wpos, w(pc + ".bias"), padding=k_pos // 2, groups=groups)
    if k_pos % 2 == 0:
        p = p[:, :, :-1]
    x = x + F.gelu(p.transpose(1, 2))
    if taps is not None:
        taps["after_pos_conv"] = flat(x)
    B, T, d = x.shape[0], x.shape[1], hidden // heads
    split = lambda t: t.reshape(B, T, heads, d).transpose(1, 2)                       # [B, heads, T, d]
    for l in range(cfg["num_hidden_layers"]):
        pre = f"encoder.layers.{l}"
        y = ln(x, pre + ".layer_norm", eps)
        q, k, vv = (split(lin(y, f"{pre}.attention.{n}_proj")) for n in "qkv")
        a = torch.softmax(q @ k.transpose(-1, -2) / d ** 0.5, dim=-1)
        if taps is not None and l == 0:
            taps["attention_0"] = a                                                   # softmax weights [B, heads, T, T]: how peaked a test case is
        a = a @ vv
        x = x + lin(a.transpose(1, 2).reshape(B, T, hidden), pre + ".attention.out_proj")
        y = F.gelu(lin(ln(x, pre + ".final_layer_norm", eps), pre + ".feed_forward.intermediate_dense"))
        x = x + lin(y, pre + ".feed_forward.output_dense")
        if taps is not None and l == 0:
            taps["layer_0"] = flat(x)
    return ln(x, "encoder.layer_norm", eps)
