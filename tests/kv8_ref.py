"""oracle.lm.forward_rows restated with a hook on the new tokens' K (after RoPE)
and V before they join the cache: the reference of an LM whose KV cache stores
quantised rows.  With the identity hook it is oracle.lm.forward_rows bit for
bit (tests/test_kv8_cpu.py pins that), with vibevoice_amd.weights.fake_quantize_kv
it is the reference of the FP8 KV cache: every key and value attention reads,
the pass's own tokens included, is a dequantised stored value."""
import torch
import torch.nn.functional as F

from oracle.lm import _rot, rms, rope_cos_sin


def forward_rows(sd, cfg, x, kvs, commit=True, kv_hook=lambda t: t):
    H = cfg["hidden_size"]
    nh, nkv = cfg["num_attention_heads"], cfg["num_key_value_heads"]
    d = cfg.get("head_dim") or H // nh
    eps, theta = cfg["rms_norm_eps"], cfg["rope_theta"]
    R, T, _ = x.shape
    h = x
    new_kv = [([None] * cfg["num_hidden_layers"], [None] * cfg["num_hidden_layers"]) for _ in range(R)]
    for li in range(cfg["num_hidden_layers"]):
        p = f"layers.{li}."
        a = rms(h, sd[p + "input_layernorm.weight"], eps)
        q = F.linear(a, sd[p + "self_attn.q_proj.weight"], sd[p + "self_attn.q_proj.bias"])
        k = F.linear(a, sd[p + "self_attn.k_proj.weight"], sd[p + "self_attn.k_proj.bias"])
        v = F.linear(a, sd[p + "self_attn.v_proj.weight"], sd[p + "self_attn.v_proj.bias"])
        outs = []
        for r in range(R):
            L0 = kvs[r].length()
            pos = torch.arange(L0, L0 + T, device=x.device)
            cos, sin = rope_cos_sin(pos, d, theta, x.dtype)
            qr = q[r].view(T, nh, d).transpose(0, 1)
            kr = k[r].view(T, nkv, d).transpose(0, 1)
            vr = v[r].view(T, nkv, d).transpose(0, 1)
            qr = qr * cos + _rot(qr) * sin
            kr = kr * cos + _rot(kr) * sin
            kr, vr = kv_hook(kr), kv_hook(vr)               # what the cache stores for the new tokens
            kc = kr if kvs[r].k[li] is None else torch.cat([kvs[r].k[li], kr], dim=1)
            vc = vr if kvs[r].v[li] is None else torch.cat([kvs[r].v[li], vr], dim=1)
            new_kv[r][0][li], new_kv[r][1][li] = kc, vc
            rep = nh // nkv
            kk = kc.repeat_interleave(rep, dim=0)
            vv = vc.repeat_interleave(rep, dim=0)
            s = torch.matmul(qr, kk.transpose(1, 2)) * d ** -0.5
            mask = torch.full((T, kc.shape[1]), float("-inf"), device=x.device)
            mask = torch.triu(mask, diagonal=L0 + 1)
            pw = F.softmax(s.float() + mask, dim=-1).to(x.dtype)
            outs.append(torch.matmul(pw, vv).transpose(0, 1).reshape(T, nh * d))
        o = F.linear(torch.stack(outs), sd[p + "self_attn.o_proj.weight"])
        h = h + o
        a = rms(h, sd[p + "post_attention_layernorm.weight"], eps)
        m = F.linear(F.silu(F.linear(a, sd[p + "mlp.gate_proj.weight"])) * F.linear(a, sd[p + "mlp.up_proj.weight"]),
                     sd[p + "mlp.down_proj.weight"])
        h = h + m
    if commit:
        for r in range(R):
            kvs[r].k, kvs[r].v = new_kv[r]
    return rms(h, sd["norm.weight"], eps)
