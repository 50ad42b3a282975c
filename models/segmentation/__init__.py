from vstnet_amd.segformer import SegFormer  # noqa: F401,E402  (the device segmenter behind --auto_seg)
