"""Dataset readers with the reference's module names (`SOccDPT.datasets.bdd_helper`, `SOccDPT.datasets.bengaluru_driving_dataset`)."""

# why `-dt idd` and `-dt idd+bdd` are refused by the training and evaluation entry points
IDD_UNSUPPORTED = ("-dt idd / idd+bdd: the IDD label set has more than three classes, and the engine's projection stage -- like the reference's own "
                   "(model/SOccDPT.py:343-349, which reshapes the point cloud with num_classes == 3) -- is built for exactly three; only the 3-class "
                   "Bengaluru layout (-dt bdd) can be trained and evaluated with SOccDPT_V3")
