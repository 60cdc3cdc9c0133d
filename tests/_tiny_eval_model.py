"""The tiny model the solver's evaluation-loop tests score: labels of FakeImageNet's first samples spread over the top ranks."""
import torch


def tiny_eval_model(n=8):
    """The tiny model of the solver's distributed test, with the biases of the `n` samples' label classes lifted to the top of
    the logits in steps: the images are noise, so every sample sees nearly the same logits, and the eight labels then sit at ranks
    around 0 .. 7 -- on both sides of k = 1 and k = 5 -- instead of all being misses."""
    from robustart_amd.train import cls_solver as S
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3, stride=4), torch.nn.ReLU(), torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten(),
                            torch.nn.Linear(4, 1000)).eval()
    x, y = S.FakeImageNet(n, 224).batch(range(n), 'cpu')
    mean, std = torch.tensor(S.IMAGENET_MEAN).view(1, 3, 1, 1), torch.tensor(S.IMAGENET_STD).view(1, 3, 1, 1)
    with torch.no_grad():
        lg = m((x.permute(0, 3, 1, 2).float() / 255.0 - mean) / std)
        top, spread = lg.max(), lg.std()
        for i, lab in enumerate(y.tolist()):
            m[-1].bias[lab] += (top - lg[:, lab].mean()) + spread * (0.3 - 0.1 * i)
    assert len(set(y.tolist())) == n
    for p in m.parameters():
        p.requires_grad_(False)
    return m
