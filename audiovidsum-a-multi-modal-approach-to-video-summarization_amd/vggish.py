"""VGGish on the MI355X: the third branch of the reference's audio extractor.

The reference obtains it with ``torch.hub.load("harritaylor/torchvggish", "vggish")`` (features/extractors.py:188) —
a network fetch that is never attempted here — and calls it at :216 (dead code at run time, Q5).  This
module supplies

  * a parameter container with torchvggish's module tree and state-dict keys (``features.{0,3,6,8,11,13}``,
    ``embeddings.{0,2,4}``, ``pproc.pca_eigen_vectors`` / ``pproc.pca_means``): a checkpoint of the hub model loads
    with ``load_state_dict``; without one the weights are a seeded synthetic init;
  * the forward pass through libavsum_hip.so: log-mel front end (fp64-MFMA DFT of the 25 ms / 10 ms frames read in
    place, magnitude -> 64-band mel -> ln(x + 0.01)), six 3x3 convolutions + ReLU with four 2x2 max-pools on NHWC
    (the (h, w, c) flatten torchvggish wants is then a plain view), three Linear + ReLU, PCA + 8-bit quantiser.

The algorithm is third-party and absent from /root/reference: restated from its published sources [3P-memory],
parity unpinned (oracle/vggish.py is the CPU restatement the GPU tests compare against).
"""
import math

import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._header import load as _load_header

_H = _load_header().constants     # the sizes avs_vggish_examples_f32 shares (include/avsum_hip.h)
SAMPLE_RATE = 16000
WINDOW, HOP, FFT_LEN = _H["AVS_VGG_WINDOW"], _H["AVS_VGG_HOP"], 512   # 400, 160
NUM_BINS, NUM_MEL = _H["AVS_VGG_BINS"], 64                            # 257 = FFT_LEN // 2 + 1
MEL_MIN_HZ, MEL_MAX_HZ = 125.0, 7500.0
EXAMPLE_FRAMES = _H["AVS_VGG_FRAMES"]                                 # 96
QUANT_MIN, QUANT_MAX = -2.0, 2.0


def _hertz_to_mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def vggish_mel_matrix():
    """float64 [257, 64]: triangles in mel space between 125 and 7500 Hz, DC row zeroed."""
    bins_mel = _hertz_to_mel(np.linspace(0.0, SAMPLE_RATE / 2.0, NUM_BINS))
    edges = np.linspace(_hertz_to_mel(MEL_MIN_HZ), _hertz_to_mel(MEL_MAX_HZ), NUM_MEL + 2)
    w = np.empty((NUM_BINS, NUM_MEL))
    for i in range(NUM_MEL):
        lower, center, upper = edges[i:i + 3]
        w[:, i] = np.maximum(0.0, np.minimum((bins_mel - lower) / (center - lower), (upper - bins_mel) / (upper - center)))
    w[0, :] = 0.0
    return w


class VGGishFrontEnd:
    """Device constants + launch sequence of waveform -> log-mel examples [n, 96, 64]."""

    _cache = {}

    def __init__(self, device):
        n = np.arange(WINDOW)
        window = 0.5 - 0.5 * np.cos(2.0 * np.pi / WINDOW * n)          # "periodic Hann" of mel_features.py
        k = np.arange(NUM_BINS)[None, :]
        ang = 2.0 * math.pi * ((n[:, None] * k) % FFT_LEN) / FFT_LEN   # 512-point rFFT of the zero-padded frame
        bt = np.zeros((WINDOW, 576), dtype=np.float64)                 # columns: 257 re | 257 im | padding to 64s
        bt[:, :NUM_BINS] = np.cos(ang) * window[:, None]
        bt[:, NUM_BINS:2 * NUM_BINS] = -np.sin(ang) * window[:, None]
        self.basis_t = torch.from_numpy(bt).to(device)
        fb = vggish_mel_matrix().astype(np.float32)
        nz = fb > 0
        self.fb = torch.from_numpy(fb).to(device)
        self.fb_lo = torch.from_numpy(np.where(nz.any(0), nz.argmax(0), 0).astype(np.int32)).to(device)
        self.fb_hi = torch.from_numpy(np.where(nz.any(0), NUM_BINS - nz[::-1].argmax(0), 0).astype(np.int32)).to(device)

    @classmethod
    def get(cls, device):
        key = str(device)
        if key not in cls._cache:
            cls._cache[key] = cls(device)
        return cls._cache[key]

    @staticmethod
    def num_frames(t):
        return 0 if t < WINDOW else 1 + (t - WINDOW) // HOP

    @classmethod
    def num_examples(cls, t):
        f = cls.num_frames(t)
        return 0 if f < EXAMPLE_FRAMES else 1 + (f - EXAMPLE_FRAMES) // EXAMPLE_FRAMES

    def log_mel(self, wave):
        """wave fp32 [T] on device -> fp32 [frames, 64] = ln(|STFT| . mel + 0.01)."""
        frames = self.num_frames(wave.numel())
        if frames == 0:
            return torch.zeros((0, NUM_MEL), dtype=torch.float32, device=wave.device)
        spec = ops.stft_f64(wave.contiguous(), frames, HOP, WINDOW, self.basis_t, 2 * NUM_BINS)
        return ops.power_mel(spec, NUM_BINS, self.fb, self.fb_lo, self.fb_hi, 3)

    def examples(self, wave):
        """-> fp32 [n, 96, 64]: non-overlapping 0.96 s patches (vggish_input.waveform_to_examples)."""
        n = self.num_examples(wave.numel())
        lm = self.log_mel(wave)
        return lm[:n * EXAMPLE_FRAMES].view(n, EXAMPLE_FRAMES, NUM_MEL)


class _Postprocessor(nn.Module):
    def __init__(self):
        super().__init__()
        self.pca_eigen_vectors = nn.Parameter(torch.empty((128, 128)), requires_grad=False)
        self.pca_means = nn.Parameter(torch.empty((128, 1)), requires_grad=False)


class VGGish(nn.Module):
    """``vggish = VGGish(); vggish(waveform_numpy, fs)`` -> [n, 128] (squeezed) like the torch.hub model."""

    def __init__(self, postprocess=True, preprocess=True):
        super().__init__()
        layers, cin = [], 1
        for v in (64, "M", 128, "M", 256, 256, "M", 512, 512, "M"):
            if v == "M":
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            else:
                layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
                cin = v
        self.features = nn.Sequential(*layers)
        self.embeddings = nn.Sequential(nn.Linear(512 * 4 * 6, 4096), nn.ReLU(True), nn.Linear(4096, 4096),
                                        nn.ReLU(True), nn.Linear(4096, 128), nn.ReLU(True))
        self.pproc = _Postprocessor()
        self.postprocess, self.preprocess = postprocess, preprocess
        # Synthetic init (the released weights are a download): variance-preserving layers, an orthogonal PCA basis
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.kaiming_normal_(m.weight, mode="fan_in", nonlinearity="relu")
                nn.init.normal_(m.bias, std=0.05)
        q, _ = torch.linalg.qr(torch.randn(128, 128))
        self.pproc.pca_eigen_vectors.data.copy_(q)
        self.pproc.pca_means.data.normal_(std=0.5)
        self.eval()
        self._key, self._w = None, None

    def _prepare(self, dev):
        key = tuple((p.data_ptr(), p._version) for p in self.parameters()) + (str(dev),)
        if self._w is not None and key == self._key:
            return self._w
        w = {"convs": [], "fcs": []}
        for m in self.features:
            if isinstance(m, nn.Conv2d):
                wt = m.weight.detach().float().to(dev)
                o, i, kh, kw = wt.shape
                ci = max(i, 4)                       # the contraction reads 16-byte channel runs: pad cin 1 -> 4
                k = torch.zeros((o, kh, kw, ci), dtype=torch.float32, device=dev)
                k[..., :i] = wt.permute(0, 2, 3, 1)
                w["convs"].append((k.reshape(o, -1).contiguous(), m.bias.detach().float().to(dev).contiguous(), ci))
            elif isinstance(m, nn.MaxPool2d):
                w["convs"].append(None)
        for m in self.embeddings:
            if isinstance(m, nn.Linear):
                w["fcs"].append((m.weight.detach().float().to(dev).contiguous(),
                                 m.bias.detach().float().to(dev).contiguous()))
        e = self.pproc.pca_eigen_vectors.detach().double().cpu()
        mu = self.pproc.pca_means.detach().double().cpu()
        w["pca"] = (e.float().to(dev).contiguous(), (-(e @ mu)).reshape(-1).float().to(dev).contiguous())
        self._w, self._key = w, key
        return w

    def embed_examples(self, examples):
        """examples fp32 [n, 96, 64] on device -> fp32 [n, 128] (before the post-processor)."""
        n = examples.shape[0]
        dev = examples.device
        if n == 0:
            return torch.zeros((0, 128), dtype=torch.float32, device=dev)
        w = self._prepare(dev)
        x = torch.zeros((n, EXAMPLE_FRAMES, NUM_MEL, 4), dtype=torch.float32, device=dev)
        x[..., 0] = examples
        for layer in w["convs"]:
            nb, h, ww, _ = x.shape
            if layer is None:
                x = ops.pool2d(x, "max", 2, 2, 0, torch.empty((nb, h // 2, ww // 2, x.shape[3]), dtype=x.dtype, device=dev))
            else:
                wt, bias, _ = layer
                x = ops.conv2d(x, wt, 3, 3, 1, 1, torch.empty((nb, h, ww, wt.shape[0]), dtype=x.dtype, device=dev),
                               bias, ops.ACT_RELU)
        x = x.reshape(n, -1)   # NHWC flatten == torchvggish's transpose(1,3).transpose(1,2).view(n,-1)
        for wt, bias in w["fcs"]:
            x = ops.linear(x, wt, bias, ops.ACT_RELU)
        return x

    def post(self, emb):
        """PCA -> clip to [-2, 2] -> quantise to 0..255 (float)."""
        e, b = self._prepare(emb.device)["pca"]
        if emb.shape[0] == 0:
            return emb
        return ops.quantize(ops.linear(emb.contiguous(), e, b), QUANT_MIN, QUANT_MAX, 255.0 / (QUANT_MAX - QUANT_MIN))

    @torch.no_grad()
    def embed_shots(self, tables, out=None):
        """tables = audio.MelPlan.shot_tables(...) on the device -> fp32 [nshot, 128] (or into `out`, rows of unit column
        stride): per shot the mean over its examples of what forward(clamped shot) returns (post-processed when
        self.postprocess), zeros for a shot without examples.  The examples of all shots come from one
        avs_vggish_examples_f32 call, then one embed_examples and one post."""
        nshot = tables.ex_seg.numel() - 1
        dev = tables.waves.device
        if out is None:
            out = torch.empty((nshot, 128), dtype=torch.float32, device=dev)
        if tables.ex_start.numel() == 0 or nshot == 0:
            return out.zero_()
        fe = VGGishFrontEnd.get(dev)
        examples = ops.vggish_examples(tables.waves, tables.ex_start, fe.basis_t, fe.fb, fe.fb_lo, fe.fb_hi)
        emb = self.embed_examples(examples)
        if self.postprocess:
            emb = self.post(emb)
        return ops.segment_mean(emb.contiguous(), tables.ex_seg, out)

    @torch.no_grad()
    def forward(self, x, fs=None):
        if not torch.cuda.is_available():
            raise RuntimeError("avsum_amd needs an MI355X (HIP device); there is no CPU fallback")
        dev = torch.device("cuda", torch.cuda.current_device())
        if self.preprocess:
            if not isinstance(x, np.ndarray):
                raise AttributeError("VGGish takes a numpy waveform (and its sample rate) when preprocess=True")
            if fs is not None and fs != SAMPLE_RATE:
                from .audio import resample_to
                x = resample_to(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev), fs, SAMPLE_RATE)
            else:
                if x.ndim > 1:
                    x = x.mean(axis=1)
                x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
            examples = VGGishFrontEnd.get(dev).examples(x)
        else:
            examples = torch.as_tensor(x, dtype=torch.float32).to(dev).reshape(-1, EXAMPLE_FRAMES, NUM_MEL)
        emb = self.embed_examples(examples.contiguous())
        if self.postprocess:
            emb = self.post(emb)
        return torch.squeeze(emb)
