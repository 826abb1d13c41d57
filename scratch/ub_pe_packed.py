"""Times the plain and the counted PE MLP entries at the benchmark's shape (32 clouds x 2048 points, ball query of the fine stage)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "openvino-sam-6d_amd"))
import torch
from sam6d_hip import _lib, pem, synth
dev = torch.device("cuda:0")
W = pem.PemWeights(synth.make_pem_weights(1), dev)
d = synth.config2_inputs(B=32, seed=1)
for name in ("dense_pm", "dense_po"):
    pts = d[name].to(dev).contiguous()
    with torch.cuda.device(dev):
        idx12, cnt12 = pem.pe_group(pts)
    B, N, _ = pts.shape
    for k in range(2):
        idx, cnt = idx12[k], cnt12[k]
        S = idx.shape[2]
        L = W.pe["mlp"][k]
        args = [L[i][j].data_ptr() for i in range(3) for j in ("w", "scale", "shift")]
        st = torch.cuda.current_stream().cuda_stream
        res = {}
        for wg in (0, 512):
            outs = []
            for entry, tail in (("sam6d_pe_mlp_max_wg", [wg]), ("sam6d_pe_mlp_max_counted", [wg, cnt.data_ptr()])):
                out = torch.zeros(B * N, 128, device=dev)
                f = lambda: _lib.call(entry, pts.data_ptr(), idx.data_ptr(), B, N, S, *args, out.data_ptr(), 128, 0, *tail, st)
                for _ in range(5): f()
                torch.cuda.synchronize()
                a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(50): f()
                b.record(); torch.cuda.synchronize()
                res[(wg, entry)] = a.elapsed_time(b) * 1000 / 50
                outs.append(out)
            assert torch.equal(outs[0], outs[1]), "counted differs"
        print("%s S %d mean cnt %.1f | wg 0: plain %.1f us counted %.1f us | wg 512: plain %.1f us counted %.1f us" % (
            name, S, float(cnt.float().mean()), res[(0, "sam6d_pe_mlp_max_wg")], res[(0, "sam6d_pe_mlp_max_counted")],
            res[(512, "sam6d_pe_mlp_max_wg")], res[(512, "sam6d_pe_mlp_max_counted")]), flush=True)
