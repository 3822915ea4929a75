"""One 100 MB decompress_device call (textgen(100,000,000, seed 1), level 9), checked: the program that profiles/dec_device/ traces with
rocprofv3 --kernel-trace --memory-copy-trace --stats -- python tools/dec_device_prof.py (the trace also holds the compress that makes the stream)."""
import sys, numpy as np, torch
sys.path.insert(0, "tests"); sys.path.insert(0, ".")
torch.zeros(1, device="cuda")
import importlib, recipes
pkg = importlib.import_module("compressjs-flattened_amd")
data = recipes.textgen(100000000, 1)
s = pkg.Bzip2.compressFile(data, None, 9)
d_in = torch.from_numpy(np.ascontiguousarray(s)).cuda(); d_out = torch.empty(data.size, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
assert pkg.decompress_device(d_in.data_ptr(), s.size, d_out.data_ptr(), d_out.numel()) == data.size
torch.cuda.synchronize()
print("one call ok")
