"""Weight packing: reference-layout parameters -> the operand images of the HIP kernels (done once per load_state_dict / device move).
No arithmetic of the forward happens here, and nothing here reads the engine's switches.

  * every conv + eval-mode BatchNorm pair is folded:  w' = w * gamma/sqrt(var+eps),  b' = beta - mean*gamma/sqrt(var+eps)
    (reference applies nn.Conv2d then nn.BatchNorm2d, e.g. interformer_pureMulti.py:53-60); folding is done in
    float64 and rounded once to fp32.
  * conv weights go to the "k4" layout  [tap][cin/4][cout_pad][4]  consumed by i2r_conv (include/i2r_hip.h).
  * ConvTranspose2d(k4,s2,p1) is split into its four output-parity 2x2 convolutions.
  * encoder matrices ([out][in], zero-padded to multiples of 16) are stored fragment-packed: every 16x16 block as the MFMA
    A-operand image in lane order (pack_frag), so one 64-lane 16-byte load is 1 KB contiguous.
"""
import torch


def _m16(c):
    return (c + 15) // 16 * 16


def _r16(c):
    """Channel count -> row width of an activation / padded width of a weight matrix: the next multiple of 16 whose number of
    16-channel fragments the conv kernels can split (a multiple of 3, 4 or 5: conv_split, csrc/i2r_conv_plan.h).  Every width of the shipped
    models is its own image (48, 64, 80 = 78 padded, 96, 160, 192, 256, 320, 384, 624, ...); 16 and 32 (HRNet-W32's first branch, W18)
    become 48 with zero weights and zero activations in the pad channels."""
    n = (c + 15) // 16
    while not any(n % k == 0 for k in (3, 4, 5)):
        n += 1
    return 16 * n


def fold_bn(w, bn, conv_bias=None, eps=1e-5):
    """w [Cout, ...] fp32 CPU; bn = (gamma, beta, mean, var) or None -> (w', b') float64."""
    w = w.double()
    cout = w.shape[0]
    b = conv_bias.double() if conv_bias is not None else torch.zeros(cout, dtype=torch.float64)
    if bn is not None:
        gamma, beta, mean, var = [t.double() for t in bn]
        scale = gamma / torch.sqrt(var + eps)
        w = w * scale.view(-1, *([1] * (w.dim() - 1)))
        b = (b - mean) * scale + beta
    return w, b


def pack_k4(w_taps, cin_pad, cout_pad):
    """w_taps [ntaps, cin, cout] -> fp32 [ntaps, cin_pad/4, cout_pad, 4] (zero padded)."""
    nt, cin, cout = w_taps.shape
    full = torch.zeros(nt, cin_pad, cout_pad, dtype=torch.float64)
    full[:, :cin, :cout] = w_taps
    return full.view(nt, cin_pad // 4, 4, cout_pad).permute(0, 1, 3, 2).contiguous().float()


PRECISIONS = {"fp32": 0, "bf16": 1, "fp16": 2}


def pack_frag(m):
    """[rows, cols] (both multiples of 16) -> MFMA A-operand images in lane order (csrc/i2r_encoder.hip header):
    packed[((rb*KC + c)*64 + l)*4 + r] = m[16 rb + (l & 15)][16 c + 4 (l >> 4) + r]; one 64-lane 16-byte load = 1 KB contiguous."""
    rows, cols = m.shape
    assert rows % 16 == 0 and cols % 16 == 0
    v = m.reshape(rows // 16, 16, cols // 16, 4, 4)              # [rb, li, c, g, r]
    return v.permute(0, 2, 3, 1, 4).contiguous().reshape(rows, cols)  # [rb, c, g, li, r]


def pack_frag32(m):
    """[rows, cols] (rows a multiple of 16, cols of 32) -> A-operand images of the 32-deep 16-bit MFMA in lane order (csrc/i2r_conv1x1_lp.hip):
    packed[((rb*KC + c)*64 + l)*8 + r] = m[16 rb + (l & 15)][32 c + 8 (l >> 4) + r]; one 64-lane 16-byte load = 1 KB contiguous."""
    rows, cols = m.shape
    assert rows % 16 == 0 and cols % 32 == 0
    v = m.reshape(rows // 16, 16, cols // 32, 4, 8)              # [rb, li, c, g, r]
    return v.permute(0, 2, 3, 1, 4).contiguous().reshape(rows, cols)  # [rb, c, g, li, r]


def pack_k8(w_taps, cin_pad, cout_pad, tdtype):
    """w_taps [ntaps, cin, cout] -> 16-bit [ntaps, g8_pad, cout_pad, 8] (cin zero-padded to whole 32-channel MFMA steps)."""
    nt, cin, cout = w_taps.shape
    g8_pad = (cin_pad // 8 + 3) // 4 * 4
    full = torch.zeros(nt, g8_pad * 8, cout_pad, dtype=torch.float64)
    full[:, :cin, :cout] = w_taps
    return full.float().to(tdtype).view(nt, g8_pad, 8, cout_pad).permute(0, 1, 3, 2).contiguous()


def winograd_weights(wf):
    """[cout, cin, 3, 3] float64 -> U = G g G^T per (cout, cin) as [16, cin, cout] (position p = 4 i + j), the weight side of
    Winograd F(2x2, 3x3) (csrc/i2r_conv_wino.hip); done in float64 and rounded once to fp32 by pack_k4"""
    G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64)
    U = torch.einsum("ia,ocab,jb->ijco", G, wf.double(), G)
    return U.reshape(16, wf.shape[1], wf.shape[0])


class PackedConv:
    __slots__ = ("w", "bias", "cin", "cin_pad", "cout", "cout_pad", "taps", "iy0", "ix0", "stride", "ksize", "dtype", "w_wino", "w_frag", "w_lp1")

    def __init__(self, w, bias, cin, cout, taps, iy0, ix0, stride, ksize, cin_pad=None, dtype=0):
        self.w, self.bias = w, bias
        self.cin, self.cin_pad = cin, (w.shape[1] * 4 if cin_pad is None else cin_pad)
        self.cout, self.cout_pad = cout, w.shape[2]
        self.taps, self.iy0, self.ix0, self.stride, self.ksize = taps, iy0, ix0, stride, ksize
        self.dtype = dtype
        self.w_wino = None  # fp32 3x3 stride-1 convs: the Winograd-domain weights [16][cin/4][cout_pad][4] (Packer.conv)
        self.w_lp1 = None   # 16-bit 1x1 stride-1 convs: the [cout_pad, cin_pad] matrix as 16-bit MFMA A-operand fragments for i2r_conv1x1_lp
        self.w_frag = None  # fp32 1x1 convs of layer1: the [cout, cin] matrix as MFMA A-operand fragments (pack_frag) for i2r_conv1x1_pair


class Packer:
    def __init__(self, sd, device, precision="fp32"):
        self.sd = {k: v.detach().to("cpu") for k, v in sd.items()}
        self.device = device
        self.dtype = PRECISIONS[precision]  # MFMA operand type of the conv kernels (accumulation / storage stay fp32)

    def _pc(self, w_taps, bias, cin, cout, taps, iy0, ix0, stride, ksize):
        """PackedConv in this packer's MFMA operand type."""
        cin_pad, cout_pad = _r16(cin), _r16(cout)
        if self.dtype == 0:
            w = pack_k4(w_taps, cin_pad, cout_pad)
        else:
            w = pack_k8(w_taps, cin_pad, cout_pad, torch.bfloat16 if self.dtype == 1 else torch.float16)
        pc = PackedConv(self._dev(w), bias, cin, cout, taps, iy0, ix0, stride, ksize, cin_pad=cin_pad, dtype=self.dtype)
        if self.dtype != 0 and ksize == 1 and stride == 1 and w_taps.shape[0] == 1 and cin_pad >= 64 and any((cout_pad // 16) % k == 0 for k in (3, 4, 5, 6)):
            full = torch.zeros(cout_pad, (cin_pad + 31) // 32 * 32, dtype=torch.float64)
            full[:cout, :cin] = w_taps[0].t()
            pc.w_lp1 = self._dev(pack_frag32(full).float().to(torch.bfloat16 if self.dtype == 1 else torch.float16))
        return pc

    def _bn(self, key):
        if key is None:
            return None
        s = self.sd
        return (s[key + ".weight"], s[key + ".bias"], s[key + ".running_mean"], s[key + ".running_var"])

    def _dev(self, t):
        return t.contiguous().to(self.device)

    def _bias(self, b, n):
        """bias b zero-padded to the n padded output channels: filled in float64, rounded once to fp32, on the device"""
        bias = torch.zeros(n, dtype=torch.float64)
        bias[:b.shape[0]] = b
        return self._dev(bias.float())

    def conv(self, conv_key, bn_key=None, stride=1, eps=1e-5):
        w = self.sd[conv_key + ".weight"]
        cout, cin, kh, kw = w.shape
        assert kh == kw and kh in (1, 3)
        wf, bf = fold_bn(w, self._bn(bn_key), self.sd.get(conv_key + ".bias"), eps)
        taps = [(dy, dx) for dy in range(kh) for dx in range(kw)]
        w_taps = wf.permute(2, 3, 1, 0).reshape(kh * kw, cin, cout)
        cout_pad = _r16(cout)
        pad = kh // 2
        pc = self._pc(w_taps, self._bias(bf, cout_pad), cin, cout, taps, -pad, -pad, stride, kh)
        nfrag = cout_pad // 16
        if self.dtype == 0 and kh == 3 and stride == 1 and (nfrag % 3 == 0 or nfrag % 4 == 0):
            pc.w_wino = self._dev(pack_k4(winograd_weights(wf), _r16(cin), cout_pad))
        return pc

    def conv_cat(self, parts, eps=1e-5):
        """Sum of 1x1 convs (+BN each) over DIFFERENT inputs as ONE 1x1 conv over the channel concatenation of those inputs:
        weights concatenated along cin (in the order of `parts`: (conv_key, bn_key)), folded biases added.  Used for the first
        Bottleneck of layer1: relu(bn3(conv3(t2)) + bn_d(downsample(x))) = relu([W3' | Wd'] . [t2 ; x] + b3' + bd')."""
        mats, bias_sum, cins = [], None, []
        for conv_key, bn_key in parts:
            w = self.sd[conv_key + ".weight"]
            cout, cin, kh, kw = w.shape
            assert kh == 1 and kw == 1
            wf, bf = fold_bn(w, self._bn(bn_key), self.sd.get(conv_key + ".bias"), eps)
            mats.append(wf.reshape(cout, cin).t())  # [cin, cout]
            bias_sum = bf if bias_sum is None else bias_sum + bf
            cins.append(cin)
        assert all(c % 16 == 0 for c in cins), "concatenated inputs must keep whole 16-channel steps"
        w_taps = torch.cat(mats, 0).unsqueeze(0)  # [1, sum cin, cout]
        cout = w_taps.shape[2]
        pc = self._pc(w_taps, self._bias(bias_sum, _r16(cout)), sum(cins), cout, [(0, 0)], 0, 0, 1, 1)
        pc.w_frag = self._frag(w_taps)
        return pc

    def _frag(self, w_taps):
        """fragment-packed [cout, cin] image of a 1x1 conv for i2r_conv1x1_pair (fp32, whole 16-channel fragments), else None"""
        _, cin, cout = w_taps.shape
        if self.dtype != 0 or w_taps.shape[0] != 1 or cin % 16 or cout % 16:
            return None
        return self._dev(pack_frag(w_taps[0].t().contiguous()).float())

    def bottlenecks(self, prefix, n):
        """layer1 of HRNet / HRFormer: n Bottleneck blocks (reference hrnet.py / hrformer.py `Bottleneck`, expansion 4); the first one
        carries a 1x1 downsample on its identity path, folded into its conv3 (conv_cat)."""
        blocks = []
        for b in range(n):
            q = "%s.%d" % (prefix, b)
            blk = dict(c1=self.conv(q + ".conv1", q + ".bn1"), c2=self.conv(q + ".conv2", q + ".bn2"))
            if (q + ".downsample.0.weight") in self.sd:
                blk["c3ds"] = self.conv_cat([(q + ".downsample.0", q + ".downsample.1"), (q + ".conv3", q + ".bn3")])
            else:
                blk["c3"] = self.conv(q + ".conv3", q + ".bn3")
            for key in ("c1", "c3"):
                if key in blk:
                    w = self.sd[q + ".conv%s.weight" % key[1]]
                    wf, _ = fold_bn(w, self._bn(q + ".bn%s" % key[1]), None, 1e-5)
                    blk[key].w_frag = self._frag(wf.reshape(1, w.shape[0], w.shape[1]).permute(0, 2, 1))
            blocks.append(blk)
        return blocks

    def linear_as_conv(self, w, b):
        """[out, in] matrix + bias -> 1x1 PackedConv."""
        cout, cin = w.shape
        return self._pc(w.double().t().reshape(1, cin, cout), self._bias(b, _r16(cout)), cin, cout, [(0, 0)], 0, 0, 1, 1)

    def deconv(self, deconv_key, bn_key, eps=1e-5):
        """ConvTranspose2d(k=4, s=2, p=1) [Cin, Cout, 4, 4] (+BN) -> {(py,px): PackedConv with 2x2 taps} (k = 3, 2: fewer taps, DECONV_TAPS).

        out[2q+py] gathers in[q+iy0+dy]:  py=0: iy0=-1, ky = 3-2dy ;  py=1: iy0=0, ky = 2-2dy  (oy = 2*iy - 1 + ky).
        """
        w = self.sd[deconv_key + ".weight"]
        cin, cout, kh, kw = w.shape
        assert kh == kw and kh in self.DECONV_TAPS, "ConvTranspose2d kernel %dx%d (the reference's _get_deconv_cfg knows 2, 3, 4)" % (kh, kw)
        wf, bf = fold_bn(w.permute(1, 0, 2, 3), self._bn(bn_key), self.sd.get(deconv_key + ".bias"), eps)  # [Cout,Cin,k,k]
        bias = self._bias(bf, _r16(cout))
        out = {}
        for py in (0, 1):
            for px in (0, 1):
                (iy0, kys), (ix0, kxs) = self.DECONV_TAPS[kh][py], self.DECONV_TAPS[kh][px]
                taps = [(dy, dx) for dy in range(len(kys)) for dx in range(len(kxs))]
                w_taps = torch.stack([wf[:, :, kys[dy], kxs[dx]].t() for dy, dx in taps], 0)  # [taps, Cin, Cout]
                out[(py, px)] = self._pc(w_taps, bias, cin, cout, taps, iy0, ix0, 1, max(len(kys), len(kxs)))
        return out

    # ConvTranspose2d(k, stride 2, padding p, output_padding op) with the reference's (k, p, op) in {(4, 1, 0), (3, 1, 1), (2, 0, 0)}
    # (_get_deconv_cfg, interformer_pureMulti.py:635-646): out[o] = sum in[i] w[o + p - 2i].  Per output parity o = 2q + par, along one
    # axis: (first input offset i0 relative to q, kernel index of every tap d, i = q + i0 + d)
    DECONV_TAPS = {4: {0: (-1, (3, 1)), 1: (0, (2, 0))},
                   3: {0: (0, (1,)), 1: (0, (2, 0))},
                   2: {0: (0, (0,)), 1: (0, (1,))}}

    def stem(self, conv_key, bn_key, eps=1e-5):
        w = self.sd[conv_key + ".weight"]  # [cout, cin, 3, 3]
        cout, cin = w.shape[:2]
        wf, bf = fold_bn(w, self._bn(bn_key), None, eps)
        return dict(w=self._dev(wf.permute(2, 3, 1, 0).reshape(9, cin, cout).float()), bias=self._dev(bf.float()),
                    cin=cin, cout=cout)

    def pe_res(self, p):
        """PositionEmbeddingImage mode 'res' (position_embedding.py:14-18): conv_pre 1->3 (3x3, no bias) and torchvision resnet18
        children()[:5] = conv1 7x7-s2 3->64 + bn1 + relu + maxpool + layer1 (2 BasicBlocks of 64), then conv_end 64->d (3x3, no BN)."""
        w_pre = self.sd[p + ".conv_pre.weight"]           # [3, 1, 3, 3]
        assert tuple(w_pre.shape) == (3, 1, 3, 3)
        w7 = self.sd[p + ".res.0.weight"]                 # [64, 3, 7, 7]
        assert tuple(w7.shape) == (64, 3, 7, 7)
        wf, bf = fold_bn(w7, self._bn(p + ".res.1"), None, 1e-5)
        blocks = []
        for b in range(2):
            q = "%s.res.4.%d" % (p, b)
            blocks.append((self.conv(q + ".conv1", q + ".bn1"), self.conv(q + ".conv2", q + ".bn2")))
        return dict(w_pre=self._dev(w_pre.view(3, 9).t().contiguous().float()),               # [tap][c]
                    w7=self._dev(wf.permute(2, 3, 1, 0).reshape(49 * 3, 64).float()), bias=self._dev(bf.float()), cout=64,
                    blocks=blocks, conv_end=self.conv(p + ".conv_end"))

    def head(self, key):
        """final_layer (with bias) for i2r_head.  EXTRA.FINAL_CONV_KERNEL = 3 (padding 1; interformer.py:176-182, interformer_pureMulti.py:486-492,
        transpose_h.py:472-478): the 3x3 conv runs on the conv kernel with its outputs padded to 48 channels (zero weights: a width the kernel
        splits), and i2r_head -- the kernel that writes the boundary NCHW layout -- follows with an identity matrix and no bias (exact in fp32)."""
        w = self.sd[key + ".weight"]
        cout, cin, kh, kw = w.shape
        assert kh == kw and kh in (1, 3), "final_layer kernel %dx%d" % (kh, kw)
        if kh == 3:
            cp = 48
            assert cout <= 32
            w_taps = torch.zeros(9, cin, cp, dtype=torch.float64)
            w_taps[:, :, :cout] = w.double().permute(2, 3, 1, 0).reshape(9, cin, cout)
            taps = [(dy, dx) for dy in range(3) for dx in range(3)]
            pc = self._pc(w_taps, self._bias(self.sd[key + ".bias"], cp), cin, cp, taps, -1, -1, 1, 3)
            if self.dtype == 0:
                wf = torch.zeros(cp, cin, 3, 3, dtype=torch.float64)
                wf[:cout] = w.double()
                pc.w_wino = self._dev(pack_k4(winograd_weights(wf), _r16(cin), cp))
            eye = torch.zeros(cout, cp)
            eye[torch.arange(cout), torch.arange(cout)] = 1.0
            return dict(w=self._dev(eye), bias=self._dev(torch.zeros(cout)), cin=cp, cout=cout, conv3=pc)
        cin_pad = _r16(cin)
        wp = torch.zeros(cout, cin_pad)
        wp[:, :cin] = w.view(cout, cin)
        return dict(w=self._dev(wp), bias=self._dev(self.sd[key + ".bias"].float()), cin=cin_pad, cout=cout)

    def encoder_layer(self, p, d, dff):
        cs, fs = _r16(d), _r16(dff)
        s = self.sd

        def padm(m, r, c):
            o = torch.zeros(r, c)
            o[:m.shape[0], :m.shape[1]] = m
            return o

        def padv(v, n):
            o = torch.zeros(n)
            o[:v.shape[0]] = v
            return o

        wi, bi = s[p + ".self_attn.in_proj_weight"], s[p + ".self_attn.in_proj_bias"]
        w_in = torch.cat([padm(wi[i * d:(i + 1) * d], cs, cs) for i in range(3)], 0)
        b_in = torch.cat([padv(bi[i * d:(i + 1) * d], cs) for i in range(3)], 0)
        t = dict(
            w_in=w_in, b_in=b_in,
            w_out=padm(s[p + ".self_attn.out_proj.weight"], cs, cs), b_out=padv(s[p + ".self_attn.out_proj.bias"], cs),
            ln1_w=padv(s[p + ".norm1.weight"], cs), ln1_b=padv(s[p + ".norm1.bias"], cs),
            w1=padm(s[p + ".linear1.weight"], fs, cs), b1=padv(s[p + ".linear1.bias"], fs),
            w2=padm(s[p + ".linear2.weight"], cs, fs), b2=padv(s[p + ".linear2.bias"], cs),
            ln2_w=padv(s[p + ".norm2.weight"], cs), ln2_b=padv(s[p + ".norm2.bias"], cs))
        lp = {}
        if self.dtype != 0:
            # 16-bit copies for the 16-bit MFMA encoder, model dim padded to csp = 96 (three 32-feature MFMA steps) for d = 96 and
            # d = 78 alike; columns of every 32-block permuted to the operand order
            # new position 8g + 4*half + r  <-  column 32c + 16*half + 4g + r   (csrc/i2r_encoder.hip)
            tdt = torch.bfloat16 if self.dtype == 1 else torch.float16
            csp = 96
            assert cs <= csp and fs == 192

            def perm(m):
                rows, cols = m.shape
                v = m.view(rows, cols // 32, 2, 4, 4)          # [row, c, half, g, r]
                v = v.permute(0, 1, 3, 2, 4).reshape(rows // 16, 16, cols // 32, 4, 8)   # [rb, li, c, g, (half, r)]
                # ... and fragment-packed like the fp32 matrices: [rb][c][g][li][8] = one 1 KB contiguous load per fragment
                return v.permute(0, 2, 3, 1, 4).reshape(rows, cols).to(tdt).contiguous()
            w_in_p = torch.cat([padm(wi[i * d:(i + 1) * d], csp, csp) for i in range(3)], 0)
            b_in_p = torch.cat([padv(bi[i * d:(i + 1) * d], csp) for i in range(3)], 0)
            lp = dict(w_in_lp=perm(w_in_p), w_out_lp=perm(padm(s[p + ".self_attn.out_proj.weight"], csp, csp)),
                      w1_lp=perm(padm(s[p + ".linear1.weight"], fs, csp)), w2_lp=perm(padm(s[p + ".linear2.weight"], csp, fs)),
                      vec_lp=torch.cat([b_in_p, padv(s[p + ".self_attn.out_proj.bias"], csp), padv(s[p + ".norm1.weight"], csp),
                                        padv(s[p + ".norm1.bias"], csp), padv(s[p + ".linear1.bias"], fs), padv(s[p + ".linear2.bias"], csp),
                                        padv(s[p + ".norm2.weight"], csp), padv(s[p + ".norm2.bias"], csp)]).float())
            lp = {k: self._dev(v) for k, v in lp.items()}
        for k in ("w_in", "w_out", "w1", "w2"):
            t[k] = pack_frag(t[k])
        t = {k: self._dev(v.float()) for k, v in t.items()}
        t.update(lp)
        t.update(d=d, cs=cs, dff_pad=fs, dtype=self.dtype if lp else 0)
        return t

    @staticmethod
    def mh_width(heads, hd):
        """(hp, hs): head dim padded to a multiple of 16 (csrc/i2r_encoder_mh.hip) and the width of a q / k / v / attention-output part,
        heads*hp rounded up to a fragment count the conv kernels split (conv_split: a multiple of 3, 4 or 5 sixteen-channel blocks)"""
        hp = _m16(hd)
        f = heads * hp // 16
        while not any(f % k == 0 for k in (3, 4, 5)):
            f += 1
        return hp, 16 * f

    def _head_padded(self, d, heads, q, k, v, o):
        """The projections around i2r_mh_attention from their (weight [d, d], bias [d]) pairs, as 1x1 convs in the head-padded channel
        order: q|k (head hh's dim j at channel hh*hp + j, the k part hs further; head_dim^-0.5 folded into the q rows), v, and the
        out-proj with zero columns for the head pads.  Assembled in float64."""
        hd = d // heads
        assert hd * heads == d, "nn.MultiheadAttention: embed_dim %d must be divisible by num_heads %d" % (d, heads)
        hp, hs = self.mh_width(heads, hd)
        rows = torch.tensor([hh * hp + j for hh in range(heads) for j in range(hd)])
        wqk, bqk = torch.zeros(2 * hs, d, dtype=torch.float64), torch.zeros(2 * hs, dtype=torch.float64)
        wqk[rows], bqk[rows] = q[0].double() * float(hd) ** -0.5, q[1].double() * float(hd) ** -0.5
        wqk[hs + rows], bqk[hs + rows] = k[0].double(), k[1].double()
        wv, bv = torch.zeros(hs, d, dtype=torch.float64), torch.zeros(hs, dtype=torch.float64)
        wv[rows], bv[rows] = v[0].double(), v[1].double()
        wo = torch.zeros(d, hs, dtype=torch.float64)
        wo[:, rows] = o[0].double()
        return dict(heads=heads, hp=hp, hs=hs, d=d, cs=_r16(d), qk=self.linear_as_conv(wqk, bqk), v=self.linear_as_conv(wv, bv),
                    o=self.linear_as_conv(wo, o[1]))

    def encoder_layer_mh(self, p, d, dff, heads):
        """General form of a DETR encoder layer (any MODEL.N_HEAD, post- or pre-norm; interformer_pureMulti.py:171-243, attention.py:37-112)
        as 1x1 convs around i2r_mh_attention: q|k (head hh's dim j at channel hh*hp + j, k part hs further; head_dim^-0.5 folded into the q
        rows), v, out-proj (zero columns for the head pads), linear1, linear2 and the two LayerNorms."""
        assert self.dtype == 0, "the general encoder layer runs in fp32 (use a Packer(..., 'fp32'))"
        s = self.sd
        wi, bi = s[p + ".self_attn.in_proj_weight"], s[p + ".self_attn.in_proj_bias"]
        proj = self._head_padded(d, heads, (wi[:d], bi[:d]), (wi[d:2 * d], bi[d:2 * d]), (wi[2 * d:], bi[2 * d:]),
                                 (s[p + ".self_attn.out_proj.weight"], s[p + ".self_attn.out_proj.bias"]))
        return dict(proj, mh=True,
                    w1=self.linear_as_conv(s[p + ".linear1.weight"], s[p + ".linear1.bias"]),
                    w2=self.linear_as_conv(s[p + ".linear2.weight"], s[p + ".linear2.bias"]),
                    ln1=self.ln(p + ".norm1", d), ln2=self.ln(p + ".norm2", d))

    def window_block(self, a, d, heads):
        """MHA_ of attention.py (:494-835) under key prefix a: separate q / k / v / out projections with bias, in the head-padded channel
        order of encoder_layer_mh (head_dim^-0.5 folded into q); the relative position table is a parameter nobody reads (:780-786)"""
        assert self.dtype == 0
        s = self.sd
        return self._head_padded(d, heads, *[(s["%s.%s_proj.weight" % (a, n)], s["%s.%s_proj.bias" % (a, n)]) for n in ("q", "k", "v", "out")])

    def dw(self, conv_key, bn_key, eps=1e-5):
        """depth-wise 3x3 [C,1,3,3] (+bias) + BN -> tap-major [9][cs] weights + [cs] bias."""
        w = self.sd[conv_key + ".weight"]
        c = w.shape[0]
        assert tuple(w.shape[1:]) == (1, 3, 3)
        wf, bf = fold_bn(w, self._bn(bn_key), self.sd.get(conv_key + ".bias"), eps)
        cs = _r16(c)
        wp = torch.zeros(9, cs, dtype=torch.float64)
        wp[:, :c] = wf.view(c, 9).t()
        bp = torch.zeros(cs, dtype=torch.float64)
        bp[:c] = bf
        return dict(w=self._dev(wp.float()), bias=self._dev(bp.float()), c=c, cs=cs)

    def ln(self, key, c):
        cs = _r16(c)
        w, b = torch.zeros(cs), torch.zeros(cs)
        w[:c], b[:c] = self.sd[key + ".weight"], self.sd[key + ".bias"]
        return dict(w=self._dev(w), b=self._dev(b), c=c, cs=cs)

    HEAD_PAD = 40  # window attention: every head's channels padded to a 16-byte multiple (head_dim 39 -> 40)

    def qkv(self, p, c, heads):
        """stacked q/k/v_proj as one 1x1 conv with 3*hs outputs (q | k | v, each hs = heads*HEAD_PAD wide): head hh's dim d sits at
        channel hh*HEAD_PAD + d, pad channels have zero weights and bias (they come out exactly 0).  The hd^-0.5 scale of the
        queries (hrformer.py:780) is folded into the q rows."""
        hd, hp = c // heads, self.HEAD_PAD
        assert hd * heads == c and hp - 4 < hd <= hp
        hs = heads * hp
        W = torch.zeros(3 * hs, c, dtype=torch.float64)
        b = torch.zeros(3 * hs, dtype=torch.float64)
        rows = torch.tensor([hh * hp + d for hh in range(heads) for d in range(hd)])
        for i, n in enumerate(("q_proj", "k_proj", "v_proj")):
            sc = float(hd) ** -0.5 if i == 0 else 1.0
            W[i * hs + rows] = self.sd["%s.%s.weight" % (p, n)].double() * sc
            b[i * hs + rows] = self.sd["%s.%s.bias" % (p, n)].double() * sc
        return self.linear_as_conv(W, b)

    def attn_out(self, p, c, heads):
        """out_proj as a 1x1 conv reading the head-padded attention output (cin = heads*HEAD_PAD, zero columns for the pads)."""
        hd, hp = c // heads, self.HEAD_PAD
        cols = torch.tensor([hh * hp + d for hh in range(heads) for d in range(hd)])
        W = torch.zeros(c, heads * hp, dtype=torch.float64)
        W[:, cols] = self.sd[p + ".out_proj.weight"].double()
        return self.linear_as_conv(W, self.sd[p + ".out_proj.bias"])

    @staticmethod
    def _frag16(m, tdt):
        """[rows, cols] (multiples of 16) -> v_mfma_f32_16x16x16 A-operand images: [rows/16][cols/16][64 lanes][4] 16-bit,
        element r of lane l = m[16 rb + (l & 15)][16 cb + 4 (l >> 4) + r]  (include/i2r_hip.h, i2r_hrt_attn_block)"""
        rows, cols = m.shape
        v = m.reshape(rows // 16, 16, cols // 16, 4, 4)              # [rb, i, cb, g, r]
        return v.permute(0, 2, 3, 1, 4).contiguous().to(tdt)         # [rb, cb, g, i, r] = lane (g, i) order

    def attn_block_lp(self, p, c, heads):
        """operands of the fused 16-bit attention half of a transformer block (i2r_hrt_attn_block); r = block key prefix"""
        tdt = torch.bfloat16 if self.dtype == 1 else torch.float16
        hd, cs = c // heads, _r16(c)
        assert hd == 39
        a = p + ".attn.attn"
        wq = torch.zeros(heads, 3, 48, cs, dtype=torch.float64)
        bq = torch.zeros(heads, 3, 48, dtype=torch.float64)
        for i, n in enumerate(("q_proj", "k_proj", "v_proj")):
            sc = float(hd) ** -0.5 * 1.4426950408889634 if i == 0 else 1.0   # softmax in base 2
            W = self.sd["%s.%s.weight" % (a, n)].double() * sc
            b = self.sd["%s.%s.bias" % (a, n)].double() * sc
            for hh in range(heads):
                wq[hh, i, :hd, :c] = W[hh * hd:(hh + 1) * hd]
                bq[hh, i, :hd] = b[hh * hd:(hh + 1) * hd]
        # 32-deep MFMA fragments (pack_frag32): input channels padded to whole 32-channel k-steps
        csp = (cs + 31) // 32 * 32
        wq_p = torch.zeros(heads * 3 * 48, csp, dtype=torch.float64)
        wq_p[:, :cs] = wq.reshape(heads * 3 * 48, cs)
        ks = csp // 32
        wqkv = pack_frag32(wq_p.float()).view(heads * 3, 3, ks, 512).permute(0, 2, 1, 3).contiguous().to(tdt)  # [(h, part)][k-step][db][64 lanes x 8]
        Wo = self.sd[a + ".out_proj.weight"].double()
        wo = torch.zeros(cs, heads, 48, dtype=torch.float64)
        for hh in range(heads):
            wo[:c, hh, :hd] = Wo[:, hh * hd:(hh + 1) * hd]
        # columns (head, dim) in the kernel's k-slot order: slot 8g + 4h + r of k-step s <- column 16 (2s + h) + 4g + r (two 16-dim
        # D fragments packed into one 32-deep B operand, csrc/i2r_hrformer_lp.hip)
        wo = wo.reshape(cs, heads * 48 // 32, 2, 4, 4).permute(0, 1, 3, 2, 4).reshape(cs, heads * 48)
        wo = pack_frag32(wo.float()).to(tdt)                                         # [ob][k-step][64 lanes][8]
        bo = torch.zeros(cs)
        bo[:c] = self.sd[a + ".out_proj.bias"]
        ln = self.ln(p + ".norm1", c)
        return dict(wqkv=self._dev(wqkv), bqkv=self._dev(bq.float()), wo=self._dev(wo), bo=self._dev(bo), ln=ln, c=c, cs=cs, heads=heads,
                    dtype=self.dtype)

    def mlp_block_lp(self, p, c):
        """operands of the fused 16-bit MLP half of a transformer block (i2r_hrt_mlp_block): fc1+BN1, dw3x3+BN2, fc2+BN3 folded in
        float64, hidden dim padded to a multiple of 64 with zeros; p = block key prefix"""
        tdt = torch.bfloat16 if self.dtype == 1 else torch.float16
        cs, hid = _r16(c), 4 * c
        hp = (hid + 63) // 64 * 64
        m = p + ".mlp"
        w1, b1 = fold_bn(self.sd[m + ".fc1.weight"], self._bn(m + ".norm1"), self.sd.get(m + ".fc1.bias"))      # [hid, c, 1, 1]
        wd, bd = fold_bn(self.sd[m + ".dw3x3.weight"], self._bn(m + ".norm2"), self.sd.get(m + ".dw3x3.bias"))  # [hid, 1, 3, 3]
        w2, b2 = fold_bn(self.sd[m + ".fc2.weight"], self._bn(m + ".norm3"), self.sd.get(m + ".fc2.bias"))      # [c, hid, 1, 1]
        assert tuple(w1.shape[:2]) == (hid, c) and tuple(w2.shape[:2]) == (c, hid)
        W1 = torch.zeros(hp, cs, dtype=torch.float64)
        W1[:hid, :c] = w1.view(hid, c)
        W2 = torch.zeros(cs, hp, dtype=torch.float64)
        W2[:c, :hid] = w2.view(c, hid)
        WD = torch.zeros(9, hp, dtype=torch.float64)
        WD[:, :hid] = wd.view(hid, 9).t()

        def padv(v, n):
            o = torch.zeros(n, dtype=torch.float64)
            o[:v.shape[0]] = v
            return o.float()
        # 32-deep MFMA fragments (pack_frag32): fc1's input channels padded to whole 32-channel k-steps; fc2's hidden columns in the
        # kernel's slot order (slot 8g + 4h + r of a k-step <- hidden channel 16 (2 kstep + h) + 4g + r: a PAIR of 16-channel hidden blocks)
        csp = (cs + 31) // 32 * 32
        W1p = torch.zeros(hp, csp, dtype=torch.float64)
        W1p[:, :cs] = W1
        W2s = W2.reshape(cs, hp // 32, 2, 4, 4).permute(0, 1, 3, 2, 4).reshape(cs, hp)
        return dict(w1=self._dev(pack_frag32(W1p.float()).to(tdt)), b1=self._dev(padv(b1, hp)), wdw=self._dev(WD.float()), bdw=self._dev(padv(bd, hp)),
                    w2=self._dev(pack_frag32(W2s.float()).to(tdt)), b2=self._dev(padv(b2, cs)), ln=self.ln(p + ".norm2", c), c=c, cs=cs, hidden_pad=hp,
                    dtype=self.dtype)

    def table(self, key, rows, d):
        """[rows, 1, d] parameter (TransPose-H pos_embedding) -> [rows, cs] device table."""
        v = self.sd[key].reshape(rows, d)
        o = torch.zeros(rows, _r16(d))
        o[:, :d] = v
        return self._dev(o)
