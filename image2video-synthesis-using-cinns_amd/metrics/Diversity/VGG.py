"""Stand-in for the reference's ``metrics/Diversity/VGG.py``: the VGG-feature diversity score is not built."""


def compute_vgg_diversity(seq1):
    raise NotImplementedError("compute_vgg_diversity is not built: it needs torchvision's VGG-16 graph and ImageNet weights, which are not part "
                              "of this package (there would be nothing to pin the features against); "
                              "metrics.Diversity.I3D.compute_DTI3D_diversity is")
