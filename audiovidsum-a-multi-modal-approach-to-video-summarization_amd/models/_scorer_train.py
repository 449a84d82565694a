"""Training-mode forward + backward of AVBiLSTMModel on the MI355X (scripts/train_av_model.py:86-96).

A torch.autograd.Function whose forward and backward are sequences of libavsum_hip.so calls: torch only owns
the tensors, the RNG that draws the Dropout masks (unless the model is seeded: then the masks are counter-based,
dropout.py, computed inside libavsum_dropout.so's kernels and never stored), and (in the caller's script) AdamW.
The rows are those of V >= 1 videos, concatenated, with the device table of their row offsets: every video is its own B = 1 call of the reference
model (the reference trains with B = 1, train_av_model.py:64,86-88) - its own four recurrences, and with B = 1 the
attention is out_proj(v_proj(x)) and the query/key projections receive exactly zero gradient.  Everything
else is row-wise.  AVBiLSTMModel.forward (V = 1, seq = [0, T]) and AVBiLSTMModel.train_rows both come through here.
"""
import torch

from .. import dropout, ops

DROPOUT_P = 0.3  # models/av_model.py:11,14


class ScorerTrainFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, visual, audio, keep_v, keep_a, seq, *params):
        """visual [R, Dv], audio [R, Da], keep_* [R, hidden]; seq int64 [V + 1] on the device: the row offsets of the
        videos (starts at 0, increases, ends at R - the caller has validated it on the host).  keep_v a dropout.Draw
        (keep_a is then ignored): the masks are the counter-based ones it names, branch 0 visual and branch 1 audio -
        applied by dropout.apply, computed again by dropout.relu_bwd in the backward, held by nobody."""
        names = [n for n, _ in model.named_parameters()]
        pm = dict(zip(names, params))
        dev = visual.device
        t = visual.shape[0]
        hidden = pm["visual_fc.0.weight"].shape[0]
        e = 2 * hidden

        # both BiLSTMs = four independent recurrences: ONE launch (direction d writes fused[:, d*H:]), as in score_rows
        saved = {}
        fused = torch.empty((t, e), dtype=torch.float32, device=dev)
        hid = pm["visual_bilstm.weight_hh_l0"].shape[1]
        xproj = torch.empty((t, 16 * hid), dtype=torch.float32, device=dev)   # [v fwd | v rev | a fwd | a rev] x 4H
        whh_all = []
        col = 0
        draw = keep_v if isinstance(keep_v, dropout.Draw) else None
        for tag, x, keep, fc, lstm in (("v", visual, keep_v, "visual_fc.0.", "visual_bilstm."),
                                       ("a", audio, keep_a, "audio_fc.0.", "audio_bilstm.")):
            r = ops.linear(x, pm[fc + "weight"], pm[fc + "bias"], ops.ACT_RELU)     # Linear + ReLU
            if draw is None:
                emb = ops.mul(r, keep)                                               # Dropout (inverted scaling)
            else:
                keep = None                                                          # nothing to hold for the backward
                emb = dropout.apply(r, draw.seed, draw.p, draw.samples, int(tag == "a"), seq)
            wih = torch.cat([pm[lstm + "weight_ih_l0"], pm[lstm + "weight_ih_l0_reverse"]], 0)
            bih = torch.cat([pm[lstm + "bias_ih_l0"] + pm[lstm + "bias_hh_l0"],
                             pm[lstm + "bias_ih_l0_reverse"] + pm[lstm + "bias_hh_l0_reverse"]])
            whh_all += [pm[lstm + "weight_hh_l0"], pm[lstm + "weight_hh_l0_reverse"]]
            ops.linear(emb, wih, bih, out=xproj[:, col * 4:(col + 2 * hid) * 4])
            saved[tag] = (x, r, keep, emb, wih, col)
            col += 2 * hid
        whh = torch.stack(whh_all).contiguous()                  # [4, 4H, H]: the backward's layout
        whh_t = whh.transpose(1, 2).contiguous()                 # [4, H, 4H]: the forward's
        gates, cell = ops.lstm_train_fwd(xproj, whh_t, hid, 4, 0b1010, seq, fused, 0)
        ctx.lstm = (whh, gates, cell, hid)
        w_in, b_in = pm["attention.in_proj_weight"], pm["attention.in_proj_bias"]
        w_v, b_v = w_in[2 * e:3 * e].contiguous(), b_in[2 * e:3 * e].contiguous()
        w_o, b_o = pm["attention.out_proj.weight"], pm["attention.out_proj.bias"]
        val = ops.linear(fused, w_v, b_v)
        attn = ops.linear(val, w_o, b_o)
        hid64 = ops.linear(attn, pm["scorer.0.weight"], pm["scorer.0.bias"], ops.ACT_RELU)
        scores = ops.score_head(hid64, pm["scorer.2.weight"].reshape(-1).contiguous(), pm["scorer.2.bias"])

        ctx.names, ctx.saved, ctx.seq, ctx.e, ctx.draw = names, saved, seq, e, draw
        ctx.tail = (fused, val, attn, hid64, scores, w_v, w_o)
        ctx.pm = pm
        ctx.need_inputs = (ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        return scores

    @staticmethod
    def backward(ctx, dscores):
        pm, e = ctx.pm, ctx.e
        fused, val, attn, hid64, scores, w_v, w_o = ctx.tail
        g = {}
        dscores = dscores.contiguous().float()
        # scoring head: Sigmoid, Linear(64,1), ReLU of scorer.0
        w2 = pm["scorer.2.weight"].reshape(-1).contiguous()
        dz, dpre = ops.score_head_bwd(dscores, scores, hid64, w2)
        g["scorer.2.weight"] = ops.colsum(hid64, dz).view(1, -1)
        g["scorer.2.bias"] = ops.colsum(dz.view(-1, 1))
        g["scorer.0.weight"] = ops.grad_weight(dpre, attn)
        g["scorer.0.bias"] = ops.colsum(dpre)
        dattn = ops.grad_input(dpre, pm["scorer.0.weight"])
        # attention with a single key: out_proj(v_proj(fused))
        g["attention.out_proj.weight"] = ops.grad_weight(dattn, val)
        g["attention.out_proj.bias"] = ops.colsum(dattn)
        dval = ops.grad_input(dattn, w_o)
        gw_in = torch.empty_like(pm["attention.in_proj_weight"])
        gb_in = torch.empty_like(pm["attention.in_proj_bias"])
        ops.fill(gw_in[:2 * e], 0.0)                                   # query / key rows: exactly zero
        ops.fill(gb_in[:2 * e], 0.0)
        ops.grad_weight(dval, fused, out=gw_in[2 * e:3 * e])
        ops.colsum(dval, out=gb_in[2 * e:3 * e])
        g["attention.in_proj_weight"], g["attention.in_proj_bias"] = gw_in, gb_in
        dfused = ops.grad_input(dval, w_v)
        dinputs = {}
        whh, gates, cell, hid = ctx.lstm
        da_all = ops.lstm_bwd(dfused, 0, gates, cell, whh, hid, 4, 0b1010, ctx.seq)   # [T, 4 * 4H], one launch
        for tag, fc, lstm in (("v", "visual_fc.0.", "visual_bilstm."), ("a", "audio_fc.0.", "audio_bilstm.")):
            x, r, keep, emb, wih, col = ctx.saved[tag]
            da = da_all[:, col * 4:(col + 2 * hid) * 4]                                  # this BiLSTM's [T, 2*4H]
            gwih = ops.grad_weight(da, emb)                                             # [8H, hidden]
            gb = ops.colsum(da)
            # h_{t-1} of each direction: forward = the previous row, reverse = the next row, zero at the first step of
            # every video (never the last state of the video before it)
            hprev_f = ops.seq_shift_rows(fused, col, hid, ctx.seq, 1)
            hprev_r = ops.seq_shift_rows(fused, col + hid, hid, ctx.seq, -1)
            g[lstm + "weight_ih_l0"], g[lstm + "weight_ih_l0_reverse"] = gwih[:4 * hid], gwih[4 * hid:]
            g[lstm + "bias_ih_l0"] = g[lstm + "bias_hh_l0"] = gb[:4 * hid]
            g[lstm + "bias_ih_l0_reverse"] = g[lstm + "bias_hh_l0_reverse"] = gb[4 * hid:]
            g[lstm + "weight_hh_l0"] = ops.grad_weight(da[:, :4 * hid], hprev_f)
            g[lstm + "weight_hh_l0_reverse"] = ops.grad_weight(da[:, 4 * hid:], hprev_r)
            demb = ops.grad_input(da, wih)
            if ctx.draw is None:
                dr = ops.relu_dropout_bwd(demb, r, keep)
            else:
                dr = dropout.relu_bwd(demb, r, ctx.draw.seed, ctx.draw.p, ctx.draw.samples, int(tag == "a"), ctx.seq)
            g[fc + "weight"] = ops.grad_weight(dr, x)
            g[fc + "bias"] = ops.colsum(dr)
            dinputs[tag] = dr
        dvis = ops.grad_input(dinputs["v"], pm["visual_fc.0.weight"]) if ctx.need_inputs[0] else None
        daud = ops.grad_input(dinputs["a"], pm["audio_fc.0.weight"]) if ctx.need_inputs[1] else None
        return (None, dvis, daud, None, None, None) + tuple(g[n].reshape(pm[n].shape) for n in ctx.names)


def dropout_keep(shape, device, p=DROPOUT_P):
    """The multiplier torch's Dropout applies in training mode: 0 with probability p, else 1/(1-p)."""
    return torch.nn.functional.dropout(torch.ones(shape, dtype=torch.float32, device=device), p, True)
